"""Token files on the MI355X: the token_batch and grad_accum_fold kernels bit for bit
against their host references, gradient accumulation against one large batch (both
anchored to fp32), and the trainer end to end on a device-resident and a host-staged
corpus.  Measured values: profiles/r11_token_data.md.
"""
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1
VOCAB = 4000  # gpt2-smoke


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(cuda)


def _host_batch(corpus, starts, S, vocab):
    w = np.stack([corpus[s:s + S + 1] for s in starts]).astype(np.int64)
    ok = w < vocab
    return (torch.from_numpy(np.where(ok, w, 0)[:, :-1].copy()), torch.from_numpy(np.where(ok, w, -1)[:, 1:].copy()),
            int((~ok).sum()))


def _launch(tok, n, B, S, vocab, draw, cuda, starts=True):
    bad = torch.zeros(1, dtype=torch.int64, device=cuda)
    so = torch.full((B,), -7, dtype=torch.int64, device=cuda) if starts else None
    idx, tgt = _m().token_batch(tok, n, B, S, vocab, bad, draw, so)
    return idx.cpu(), tgt.cpu(), int(bad.item()), (so.cpu().numpy() if starts else None)


# ----------------------------------------------------------------------------- token_batch
SHAPES = [(1, 1), (3, 127), (2, 128), (5, 1023), (4, 1024)]


@pytest.mark.parametrize("B,S", SHAPES)
def test_token_batch_matches_host_reference(cuda, B, S):
    from paddle_operator_amd.data import window_starts
    rng = np.random.default_rng(B * 10000 + S)
    parities = set()
    for n in (S + 1, S + 2, 4099):
        corpus = rng.integers(0, VOCAB, n).astype(np.uint16)
        corpus[rng.integers(0, n, max(1, n // 50))] = rng.integers(VOCAB, 65536, max(1, n // 50))  # planted ids ≥ vocab
        corpus[-1] = 65535
        tok = _dev(corpus, cuda)
        for rank, m in ((0, 0), (3, 1), (1, 2**32 + 1)):
            want_s = window_starts(SEED, 0, m, rank, B, n, S)
            idx, tgt, bad, got_s = _launch(tok, n, B, S, VOCAB, (SEED, 0, m, rank), cuda)
            assert got_s.tolist() == want_s.tolist(), (n, rank, m)
            wi, wt, wb = _host_batch(corpus, want_s, S, VOCAB)
            assert torch.equal(idx, wi) and torch.equal(tgt, wt) and bad == wb, (n, rank, m)
            parities |= {int(s) & 1 for s in want_s}
            if n == S + 1:
                assert got_s.tolist() == [0] * B
        # the evaluation stream draws other windows, without starts_out too
        idx1, tgt1, _, _ = _launch(tok, n, B, S, VOCAB, (SEED, 1, 0, 0), cuda, starts=False)
        wi, wt, _ = _host_batch(corpus, window_starts(SEED, 1, 0, 0, B, n, S), S, VOCAB)
        assert torch.equal(idx1, wi) and torch.equal(tgt1, wt)
    if S > 1 or B > 1:
        assert parities == {0, 1}  # odd and even 2-byte offsets both ran


def test_token_batch_reads_the_last_token(cuda):
    """A window whose start is n − S − 1 ends on tok[n − 1] (65535 here, so it shows in bad)."""
    from paddle_operator_amd.data import window_starts
    B, S, n = 5, 1023, 4099
    corpus = np.random.default_rng(1).integers(0, VOCAB, n).astype(np.uint16)
    corpus[-1] = 65535
    m = next(m for m in range(200000) if (window_starts(SEED, 0, m, 0, B, n, S) == n - S - 1).any())
    starts = window_starts(SEED, 0, m, 0, B, n, S)
    idx, tgt, bad, got_s = _launch(_dev(corpus, cuda), n, B, S, VOCAB, (SEED, 0, m, 0), cuda)
    wi, wt, wb = _host_batch(corpus, starts, S, VOCAB)
    r = int(np.argmax(starts == n - S - 1))
    assert got_s.tolist() == starts.tolist() and tgt[r, -1] == -1 and wb >= 1
    assert torch.equal(idx, wi) and torch.equal(tgt, wt) and bad == wb


def test_token_batch_starts_only_64bit(cuda):
    from paddle_operator_amd.data import window_starts
    n, S, B = 2**33 + 7, 1024, 64
    seen = []
    for m in (0, 1, 2**32 - 1):
        so = torch.zeros(B, dtype=torch.int64, device=cuda)
        assert _m().token_batch(None, n, B, S, VOCAB, None, (SEED, 0, m, 2), so) is None
        want = window_starts(SEED, 0, m, 2, B, n, S)
        assert so.cpu().numpy().tolist() == want.tolist()
        seen.append(want)
    assert np.concatenate(seen).max() >= 2**32  # the high word takes part in the modulo


def test_token_batch_staged_equals_device(cuda):
    from paddle_operator_amd.data import window_starts
    rng = np.random.default_rng(2)
    for B, S in SHAPES:
        n = 4099
        corpus = rng.integers(0, 4400, n).astype(np.uint16)  # ≈ 9 % of the ids ≥ vocab
        starts = window_starts(SEED, 0, 5, 1, B, n, S)
        staged = np.stack([corpus[s:s + S + 1] for s in starts])
        d = _launch(_dev(corpus, cuda), n, B, S, VOCAB, (SEED, 0, 5, 1), cuda, starts=False)
        s = _launch(_dev(staged.reshape(-1), cuda), B * (S + 1), B, S, VOCAB, None, cuda, starts=False)
        assert torch.equal(d[0], s[0]) and torch.equal(d[1], s[1]) and d[2] == s[2] == int((staged >= VOCAB).sum())
        assert d[2] > 0 or S == 1


def test_token_batch_repeatable_and_counter_accumulates(cuda):
    n, B, S = 4099, 4, 1024
    corpus = np.random.default_rng(3).integers(0, 4400, n).astype(np.uint16)
    tok = _dev(corpus, cuda)
    bad = torch.zeros(1, dtype=torch.int64, device=cuda)
    a = _m().token_batch(tok, n, B, S, VOCAB, bad, (SEED, 0, 7, 0))
    one = int(bad.item())
    b = _m().token_batch(tok, n, B, S, VOCAB, bad, (SEED, 0, 7, 0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert one >= 1 and int(bad.item()) == 2 * one  # the counter adds up across launches
    c = _m().token_batch(tok, n, B, S, VOCAB, bad, (SEED, 0, 8, 0))
    assert not torch.equal(a[0], c[0])
    # full vocabulary: nothing is out of range
    bad.zero_()
    idx, tgt = _m().token_batch(tok, n, B, S, 65536, bad, (SEED, 0, 7, 0))
    assert int(bad.item()) == 0 and int(tgt.min()) >= 0 and torch.equal(idx[:, 1:], tgt[:, :-1])


def test_token_batch_rejects_what_it_cannot_run(cuda):
    tok = _dev(np.zeros(4099), cuda)
    bad = torch.zeros(1, dtype=torch.int64, device=cuda)
    for args in ((tok, 4099, 4, 4099, VOCAB, bad, (SEED, 0, 0, 0)),        # n < S + 1
                 (tok, 4099, 4, 128, 65537, bad, (SEED, 0, 0, 0)),         # vocab beyond uint16
                 (tok, 4099, 4, 128, VOCAB, bad, (SEED, 0, 0, 2**30)),     # g ≥ 2^32
                 (tok, 4099, 4, 128, VOCAB, bad, None),                    # staged: n ≠ B·(S + 1)
                 (tok, 5000, 4, 128, VOCAB, bad, (SEED, 0, 0, 0)),         # n beyond the tensor
                 (tok.to(torch.int32), 4099, 4, 128, VOCAB, bad, (SEED, 0, 0, 0))):
        with pytest.raises(RuntimeError):
            _m().token_batch(*args)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- grad_accum_fold
@pytest.mark.parametrize("n", [1, 7, 8, 4097, 2**20 + 3])
def test_grad_accum_fold_exact(cuda, n):
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(n)).bfloat16()
    a0 = torch.randn(n, generator=torch.Generator().manual_seed(n + 1)) * 4
    # sums that bf16 cannot hold: 256 + 0.5, and cancellation down to the accumulator's low bits
    g0[::3] = 0.5
    a0[::3] = 256.0
    g0[1::5] = -1.0
    a0[1::5] = 1.0 + 2.0 ** -20
    for init, emit in itertools.product((False, True), repeat=2):
        g, acc = g0.to(cuda), a0.to(cuda)
        _m().grad_accum_fold(g, acc, init, emit)
        want_acc = (torch.zeros(n) if init else a0) + g0.float()
        want_g = want_acc.bfloat16() if emit else torch.zeros(n, dtype=torch.bfloat16)
        assert torch.equal(acc.cpu().view(torch.int32), want_acc.view(torch.int32)), (init, emit)
        assert torch.equal(g.cpu().view(torch.int16), want_g.view(torch.int16)), (init, emit)
    s = a0[0] + g0[0].float()
    assert float(s) == 256.5 and float(s.bfloat16()) == 256.0  # the planted pair: a bf16 sum loses the 0.5


# ----------------------------------------------------------------------------- accumulation vs one large batch
S_ACC = 128


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))


def _cfg():
    from paddle_operator_amd.models.gpt2 import GPT2Config
    return GPT2Config.named("gpt2-smoke")  # every dropout 0


def _view(buf, s):
    return buf[s.offset:s.offset + s.numel].view(s.shape)


def _trainer_grads(tr, x, y):
    """(loss, {name: gradient}, whole gradient arena) of one step at the initial weights."""
    loss = float(tr.step(x, y).detach())
    g = tr.flat.param_grads.float() * tr.ddp.grad_scale
    torch.cuda.synchronize()
    return loss, {s.name: _view(g, s).cpu() for s in tr.flat.slots}, g.cpu()


def _fp32_grads(tr0_master, slots, x, y):
    from paddle_operator_amd.models.gpt2 import GPT2
    ref = GPT2(_cfg())  # fp32, CPU
    params = dict(ref.named_parameters())
    with torch.no_grad():
        for s in slots:
            params[s.name].copy_(_view(tr0_master, s))
    old = os.environ.get("PDO_OPS")
    os.environ["PDO_OPS"] = "torch"
    try:
        loss = ref(x.cpu(), y.cpu())
        loss.backward()
    finally:
        if old is None:
            os.environ.pop("PDO_OPS")
        else:
            os.environ["PDO_OPS"] = old
    return float(loss.detach()), {n: p.grad.float() for n, p in params.items()}


@pytest.fixture(scope="module")
def anchors(cuda):
    """Per row count R: the rows, the fp32 loss / gradients, and the single-batch
    (grad_accum = 1, B = R) trainer's loss / gradients, computed once."""
    from paddle_operator_amd.train import GPT2Trainer
    out = {}
    for R in (6, 8, 32):
        tr = GPT2Trainer(_cfg(), R, S_ACC, cuda)
        master0 = tr.opt.master.clone().cpu()
        x, y = tr.batch()
        loss_r, g_r = _fp32_grads(master0, tr.flat.slots, x, y)
        loss_1, g_1, _ = _trainer_grads(tr, x, y)
        arena_r = torch.cat([g_r[s.name].reshape(-1) for s in tr.flat.slots])
        arena_1 = torch.cat([g_1[s.name].reshape(-1) for s in tr.flat.slots])
        out[R] = dict(x=x, y=y, loss_r=loss_r, g_r=g_r, loss_1=loss_1, g_1=g_1, arena_r=arena_r, arena_1=arena_1)
        del tr
    return out


def _accum(cuda, K, anchor, fp32_acc=True):
    from paddle_operator_amd import train
    tr = train.GPT2Trainer(_cfg(), 2, S_ACC, cuda, grad_accum=K)
    assert (tr.acc is not None) == (K > 2)
    train._ACCUM_FP32[0] = fp32_acc
    try:
        loss, g, _ = _trainer_grads(tr, anchor["x"], anchor["y"])
    finally:
        train._ACCUM_FP32[0] = True
    assert tr.drop_step == tr.data_step == K and tr.opt.step_count == 1
    arena = torch.cat([g[s.name].reshape(-1) for s in tr.flat.slots])
    return loss, g, arena


@pytest.mark.parametrize("K", [4, 3])
def test_accumulation_vs_one_large_batch(cuda, anchors, K):
    """grad_accum = K × B 2 against grad_accum = 1 × B 2K on the same rows and weights:
    per parameter, rel. L2 error against fp32 ≤ 1.5 × the single-batch trainer's; the mean
    of the K micro losses equals the large-batch loss to fp32 summation error
    (tokens · 2⁻²⁴ relative).  K = 4 and 3 run the fold's init / emit sequence (acc = g,
    then g = bf16(acc + g)); K = 2 (no accumulator) runs in the end-to-end test below."""
    a = anchors[2 * K]
    loss, g, _ = _accum(cuda, K, a)
    errs = {n: (_rel(g[n], a["g_r"][n]), _rel(a["g_1"][n], a["g_r"][n])) for n in g}
    worst = max(errs, key=lambda n: errs[n][0] / errs[n][1])
    tokens = 2 * K * S_ACC
    print(f"grad_accum {K}: loss {loss:.7f} single-batch {a['loss_1']:.7f} fp32 {a['loss_r']:.7f} "
          f"(rel. diff {abs(loss - a['loss_1']) / a['loss_1']:.3e}, bound {tokens * 2.0 ** -24:.3e}); "
          f"max err ratio {errs[worst][0] / errs[worst][1]:.3f} at {worst} {errs[worst]}")
    bad = {n: (round(ea, 5), round(e1, 5)) for n, (ea, e1) in errs.items() if not ea <= 1.5 * e1}
    assert not bad, bad
    assert abs(loss - a["loss_1"]) <= tokens * 2.0 ** -24 * a["loss_1"], (loss, a["loss_1"])


def test_fp32_accumulator_not_worse_than_bf16_accumulation(cuda, anchors):
    """K = 16 × B 2: micro-batches added straight into the bf16 arena (the fold switched
    off) against the fp32 accumulator, both as errors of the whole gradient against fp32.
    The whole arena, not each parameter: one rounding of a small parameter can fall either
    way, the sum over 4 M elements shows what the accumulator is for."""
    a = anchors[32]
    _, g_acc, arena_acc = _accum(cuda, 16, a, fp32_acc=True)
    _, g_bf, arena_bf = _accum(cuda, 16, a, fp32_acc=False)
    e1, ea, eb = _rel(a["arena_1"], a["arena_r"]), _rel(arena_acc, a["arena_r"]), _rel(arena_bf, a["arena_r"])
    per = {n: (_rel(g_acc[n], a["g_r"][n]), _rel(g_bf[n], a["g_r"][n]), _rel(a["g_1"][n], a["g_r"][n])) for n in g_acc}
    print(f"K = 16 whole-gradient rel. L2 error vs fp32: single batch {e1:.5f}, fp32 accumulator {ea:.5f} "
          f"({ea / e1:.3f}×), bf16 accumulation {eb:.5f} ({eb / e1:.3f}×); per-parameter max ratio to the single "
          f"batch: accumulator {max(v[0] / v[2] for v in per.values()):.3f}, bf16 {max(v[1] / v[2] for v in per.values()):.3f}")
    assert ea <= eb, (ea, eb, e1)


# ----------------------------------------------------------------------------- trainer end to end
@pytest.fixture(scope="module")
def token_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tok")
    rng = np.random.default_rng(7)
    paths = []
    for name in ("train.bin", "val.bin"):
        rng.integers(0, VOCAB, 4099).astype("<u2").tofile(d / name)
        paths.append(str(d / name))
    return paths


def _run3(tr, batches=None):
    losses = []
    for k in range(3):
        loss = tr.step() if batches is None else tr.step(*batches[k])
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return losses


@pytest.mark.parametrize("K", [1, 2])
def test_trainer_on_token_file_equals_host_built_batches(cuda, token_files, K):
    """3 steps drawing from the device-resident corpus = 3 steps from the host-staged
    corpus = 3 steps fed the numpy-built batches through step(idx, tgt), bit for bit."""
    from paddle_operator_amd.data import TokenStream
    from paddle_operator_amd.train import GPT2Trainer
    B = 2
    kw = dict(data=token_files[0], data_seed=SEED, grad_accum=K)
    dev = GPT2Trainer(_cfg(), B, S_ACC, cuda, **kw)
    assert dev.data.placement == "device"
    l_dev = _run3(dev)
    host = GPT2Trainer(_cfg(), B, S_ACC, cuda, data_device_gb=0.0, **kw)
    assert host.data.placement == "host"
    l_host = _run3(host)
    host.close()
    ref = TokenStream(token_files[0], B, S_ACC, VOCAB, "cpu", seed=SEED)
    batches = []
    for k in range(3):
        parts = [ref.host_batch(k * K + i) for i in range(K)]
        batches.append((torch.cat([p[0] for p in parts]).to(cuda), torch.cat([p[1] for p in parts]).to(cuda)))
    fed = GPT2Trainer(_cfg(), B, S_ACC, cuda, grad_accum=K)
    l_fed = _run3(fed, batches)
    assert l_dev == l_host == l_fed, (l_dev, l_host, l_fed)
    for tr in (dev, host):
        assert tr.data_step == 3 * K
        assert torch.equal(tr.flat.params.view(torch.int16), fed.flat.params.view(torch.int16))
        assert torch.equal(tr.opt.master, fed.opt.master)
        tr.check_data()


def test_evaluate_vs_fp32_and_training_state(cuda, token_files):
    """evaluate() against the fp32 model on the same windows, within 1.5 × the error of the
    framework in bf16; no training state moves."""
    from paddle_operator_amd.data import TokenStream
    from paddle_operator_amd.models.gpt2 import GPT2
    from paddle_operator_amd.train import GPT2Trainer
    B, NB = 2, 4
    tr = GPT2Trainer(_cfg(), B, S_ACC, cuda, data=token_files[0], val_data=token_files[1], data_seed=SEED)
    tr.step()
    state = (tr.drop_step, tr.data_step, tr.opt.step_count, tr.flat.params.clone(), tr.flat.grads.clone(),
             tr.opt.master.clone(), tr.opt.m.clone(), tr.opt.v.clone())
    val = tr.evaluate(NB)
    assert val == tr.evaluate(NB)
    assert tr.model.training and (tr.drop_step, tr.data_step, tr.opt.step_count) == state[:3]
    for was, now in zip(state[3:], (tr.flat.params, tr.flat.grads, tr.opt.master, tr.opt.m, tr.opt.v)):
        assert torch.equal(was, now)
    # the same windows through the fp32 model (CPU) and the framework in bf16 (GPU, torch ops)
    ref = GPT2(_cfg()).eval()
    with torch.device(cuda):
        fw = GPT2(_cfg()).bfloat16().eval()
    for model in (ref, fw):
        params = dict(model.named_parameters())
        with torch.no_grad():
            for s in tr.flat.slots:
                params[s.name].copy_(_view(tr.opt.master, s))
    stream = TokenStream(token_files[1], B, S_ACC, VOCAB, "cpu", seed=SEED, stream=1)
    old = os.environ.get("PDO_OPS")
    os.environ["PDO_OPS"] = "torch"
    try:
        with torch.no_grad():
            lr_, lf = [], []
            for m in range(NB):
                idx, tgt, _ = stream.host_batch(m)
                lr_.append(float(ref(idx, tgt)))
                lf.append(float(fw(idx.to(cuda), tgt.to(cuda))))
    finally:
        if old is None:
            os.environ.pop("PDO_OPS")
        else:
            os.environ["PDO_OPS"] = old
    loss_r, loss_f = float(np.mean(lr_)), float(np.mean(lf))
    print(f"evaluate: hip {val:.6f} fp32 {loss_r:.6f} framework-bf16 {loss_f:.6f}; "
          f"errors {abs(val - loss_r):.3e} vs {abs(loss_f - loss_r):.3e}")
    assert abs(val - loss_r) <= 1.5 * abs(loss_f - loss_r), (val, loss_r, loss_f)
