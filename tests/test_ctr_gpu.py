"""The CTR sparse kernels (csrc/hip/ctr.hip) and the trainer built on them, on the GPU.

Exact tests run on a dyadic grid (tests/test_ctr_cpu.py asserts that fp32 and float64
agree bit for bit there, so summation order and FMA contraction cannot show); the
random-input tests use the rounding counts stated in the header of csrc/hip/ctr.hip:

  forward, L = D/4, R = 64 // L, P = ceil(S / R), V = min(R, S), CS = P - 1 + ceil(log2 V):
    wide_sum: CS;  fm: 2·CS + 1 + 3 + ceil(log2 L), relative to Σ|terms| of the
    expanded form ½ Σ_d (Σ_ij e_i·e_j − Σ_i e_i²)
  backward, a run of n lookups: g: n − 1 (n + 2 with fm), g_w: n − 1 = CG;
    acc': half an ulp + (2·CG + 1)·2⁻²⁴·g²;  w': half an ulp + (2·CG + 4)·2⁻²⁴·|lr·g/√acc'|

The helpers of this file (grid, id patterns, references) are shared with the CPU file.
"""
import math
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SENTINEL = 0x7FC12345  # a NaN pattern no kernel produces


# ----------------------------------------------------------------------------- shared helpers
def grid(gen, shape):
    """Multiples of 2⁻⁴ in [−1, 1]."""
    return torch.randint(-16, 17, tuple(shape), generator=gen).float() / 16.0


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def exact64(a32, b64):
    """An fp32 result equals a float64 one exactly."""
    return torch.equal(a32.detach().cpu().double(), b64.detach().cpu())


def _shuffled(gen, values, B, S):
    v = torch.tensor(values, dtype=torch.int64)
    assert v.numel() == B * S
    return v[torch.randperm(B * S, generator=gen)].reshape(B, S)


def id_pattern(name):
    """``(ids [B, S] int64, rows, D)`` of a named pattern; fixed seeds."""
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "distinct":  # N = 35: no multiple of 4 or of 256
        B, S, rows, D = 7, 5, 90, 16
        return torch.randperm(rows, generator=gen)[:B * S].reshape(B, S), rows, D
    if name == "hot":  # id 3 in every sample: a run of 700 over three segments, folded across two boundaries
        B, S, rows, D = 700, 2, 60, 16
        other = torch.randint(4, rows, (B,), generator=gen)
        other[:40] = torch.randint(0, 3, (40,), generator=gen)  # the run starts inside segment 0
        return torch.stack([torch.full((B,), 3), other], dim=1), rows, D
    if name == "boundary":  # sorted: 5 ×200, 9 ×56 (ends at 256), 11 ×300 (starts at 256, crosses 512), 20 ×41
        B, S, rows, D = 199, 3, 40, 8
        return _shuffled(gen, [5] * 200 + [9] * 56 + [11] * 300 + [20] * 41, B, S), rows, D
    if name == "tiny":  # N = 3, the narrowest rows
        return torch.tensor([[2], [0], [2]]), 5, 4
    if name == "wide_rows":  # D = 64: 16 lanes per row; D = 32 below: 8
        B, S, rows, D = 65, 5, 50, 64
        return torch.randint(0, rows, (B, S), generator=gen), rows, D
    if name == "d32":
        B, S, rows, D = 9, 3, 11, 32
        return torch.randint(0, rows, (B, S), generator=gen), rows, D
    if name == "d12":  # 3 lanes per row: no power of two
        B, S, rows, D = 33, 7, 40, 12
        return torch.randint(0, rows, (B, S), generator=gen), rows, D
    if name == "zipf":
        B, S, rows, D = 40, 26, 500, 16
        z = np.random.default_rng(5).zipf(1.2, size=B * S)
        return torch.from_numpy((z - 1) % rows).reshape(B, S), rows, D
    if name == "oor":  # some ids outside the table
        B, S, rows, D = 21, 6, 30, 16
        ids = torch.randint(0, rows, (B, S), generator=gen)
        bad = torch.tensor([-1, rows, rows + 5, 1 << 40, -(1 << 35)])
        pos = torch.randperm(B * S, generator=gen)[:25]
        ids.view(-1)[pos] = bad[torch.arange(25) % 5]
        return ids, rows, D
    raise KeyError(name)


PATTERNS = ["distinct", "hot", "boundary", "tiny", "wide_rows", "d32", "d12", "zipf", "oor"]


def grid_case(name, seed=0):
    """Dyadic inputs of the backward on a pattern: everything a multiple of 2⁻⁴ in [−1, 1]."""
    ids, rows, D = id_pattern(name)
    B, S = ids.shape
    gen = torch.Generator().manual_seed(1000 + seed)
    return dict(ids=ids, rows=rows, D=D, deep=grid(gen, (rows, D)), wide=grid(gen, (rows,)),
                dX=grid(gen, (B, S * D)), dlogit=grid(gen, (B,)), ssum=grid(gen, (B, D)))


def random_case(name, seed=0):
    """Random fp32 inputs of the backward on a pattern, all positive: the bounds of the
    ADAGRAD test are relative to |g|, which a sum of terms of one sign makes the same as
    Σ|terms| (up to the e·Σdlogit part of the fm term, which is S times smaller than the
    rest); ``ssum`` is the true sum of the sample's rows, as in training."""
    from paddle_operator_amd.ops.ctr import ref_ctr_lookup
    ids, rows, D = id_pattern(name)
    B, S = ids.shape
    gen = torch.Generator().manual_seed(2000 + seed)

    def pos(shape):
        return torch.rand(shape, generator=gen) * 0.75 + 0.25
    deep, wide = pos((rows, D)), pos((rows,))
    ssum = ref_ctr_lookup(ids, torch.zeros(B, 0), deep, wide, True)[3]
    return dict(ids=ids, rows=rows, D=D, deep=deep, wide=wide, dX=pos((B, S * D)), dlogit=pos((B,)), ssum=ssum,
                acc_deep=pos((rows, D)), acc_wide=pos((rows,)))


def run_lengths(ids, rows):
    flat = ids.reshape(-1)
    ok = (flat >= 0) & (flat < rows)
    return torch.unique(flat[ok], return_counts=True)


def fwd_counts(S, D):
    """(roundings of wide_sum, roundings of fm) from the header of csrc/hip/ctr.hip."""
    L = D // 4
    R = 64 // L
    P = -(-S // R)
    V = min(R, S)
    cs = P - 1 + math.ceil(math.log2(V)) if V > 1 else P - 1
    return cs, 2 * cs + 1 + 3 + (math.ceil(math.log2(L)) if L > 1 else 0)


def half_ulp32(x64):
    return 0.5 * np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)


# ----------------------------------------------------------------------------- 1, 2: ctr_fwd
FWD_SHAPES = [(40, 26, 16, 13), (3, 1, 4, 0), (65, 5, 64, 1), (33, 7, 12, 2)]


def _fwd_inputs(B, S, D, nd, gen, dyadic):
    rows = 37
    ids = torch.randint(0, rows, (B, S), generator=gen)
    if B * S > 8:
        ids.view(-1)[::7] = torch.tensor([-1, rows, 1 << 33])[torch.arange(len(ids.view(-1)[::7])) % 3]
    mk = (lambda s: grid(gen, s)) if dyadic else (lambda s: torch.randn(s, generator=gen))
    return ids, mk((B, nd)), mk((rows, D)), mk((rows,))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FWD_SHAPES)
@pytest.mark.parametrize("pad", [0, 1, 11])
def test_ctr_fwd_exact(cuda, shape, pad):
    """X is a copy (bit-equal to indexing on random tables; padding columns are zeros, as the
    header promises); on the dyadic grid wide_sum, ssum and fm equal float64."""
    from paddle_operator_amd.ops.ctr import ctr_lookup, min_ldx, padded_ldx, ref_ctr_lookup
    B, S, D, nd = shape
    K = min_ldx(S, D, nd)
    ldx = K if pad == 0 else padded_ldx(S, D, nd) if pad == 1 else K + pad
    gen = torch.Generator().manual_seed(B * 131 + S)
    for dyadic in (False, True):
        ids, dense, deep, wide = _fwd_inputs(B, S, D, nd, gen, dyadic)
        X, ws, fm, ssum = ctr_lookup(ids.to(cuda), dense.to(cuda), deep.to(cuda), wide.to(cuda), True, ldx)
        X2, ws2, fm2, ssum2 = ctr_lookup(ids.to(cuda), dense.to(cuda), deep.to(cuda), wide.to(cuda), False, ldx)
        assert fm2 is None and ssum2 is None and same_bits(X, X2) and same_bits(ws, ws2)
        Xr = ref_ctr_lookup(ids, dense, deep, wide, False, ldx)[0]
        assert X.shape == (B, ldx) and same_bits(X, Xr)
        assert not bits(X[:, K:]).any()
        if dyadic:
            _, wr, fr, sr = ref_ctr_lookup(ids, dense.double(), deep.double(), wide.double(), True)
            assert exact64(ws, wr) and exact64(ssum, sr) and exact64(fm, fr)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_ctr_fwd_random_within_rounding_count(cuda, shape):
    from paddle_operator_amd.ops.ctr import ctr_lookup, ref_ctr_lookup
    B, S, D, nd = shape
    gen = torch.Generator().manual_seed(B * 17 + D)
    ids, dense, deep, wide = _fwd_inputs(B, S, D, nd, gen, False)
    _, ws, fm, ssum = ctr_lookup(ids.to(cuda), dense.to(cuda), deep.to(cuda), wide.to(cuda), True)
    _, wr, fr, sr = ref_ctr_lookup(ids, dense.double(), deep.double(), wide.double(), True)
    ok = (ids >= 0) & (ids < deep.shape[0])
    safe = torch.where(ok, ids, torch.zeros_like(ids))
    e = deep.double()[safe].abs() * ok[..., None]
    w_abs = (wide.double()[safe].abs() * ok).sum(1)
    c_w, c_fm = fwd_counts(S, D)
    assert ((ws.cpu().double() - wr).abs() <= c_w * U * w_abs).all()
    assert ((ssum.cpu().double() - sr).abs() <= c_w * U * e.sum(1)).all()
    fm_abs = 0.5 * (e.sum(1) ** 2 + (e * e).sum(1)).sum(1)
    err = (fm.cpu().double() - fr).abs()
    print(f"fm: max err / (u·Σ|terms|) = {(err / (U * fm_abs)).max():.3f} of {c_fm}")
    assert (err <= c_fm * U * fm_abs).all()


# ----------------------------------------------------------------------------- 3: GRAD, exact
def _sentinel(shape, dev):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _grad_launch(c, fm, dev, ldx_pad=0):
    from paddle_operator_amd.ops.ctr import GRAD, ctr_sparse_step
    B, S = c["ids"].shape
    dX = c["dX"]
    if ldx_pad:  # rows of dX strided by more than S·D
        buf = torch.zeros(B, dX.shape[1] + ldx_pad)
        buf[:, :dX.shape[1]] = dX
        dX = buf.to(dev)[:, :c["dX"].shape[1]]
    else:
        dX = dX.to(dev)
    g_deep, g_wide = _sentinel((c["rows"], c["D"]), dev), _sentinel((c["rows"],), dev)
    ctr_sparse_step(c["ids"].to(dev), dX, c["dlogit"].to(dev), c["ssum"].to(dev) if fm else None,
                    (c["deep"].to(dev), c["wide"].to(dev)), (g_deep, g_wide), None, GRAD)
    return g_deep.cpu(), g_wide.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("fm", [False, True])
@pytest.mark.parametrize("name", PATTERNS)
def test_ctr_bwd_grad_exact_on_grid(cuda, name, fm):
    from paddle_operator_amd.ops.ctr import ref_run_sums
    c = grid_case(name)
    uniq, G, Gw = ref_run_sums(c["ids"], c["dX"].double(), c["dlogit"].double(), c["ssum"].double() if fm else None,
                               c["deep"].double())
    g_deep, g_wide = _grad_launch(c, fm, cuda)
    assert exact64(g_deep[uniq], G) and exact64(g_wide[uniq], Gw)
    rest = torch.ones(c["rows"], dtype=torch.bool)
    rest[uniq] = False
    assert (bits(g_deep[rest]) == SENTINEL).all() and (bits(g_wide[rest]) == SENTINEL).all()
    again = _grad_launch(c, fm, cuda)
    assert same_bits(g_deep, again[0]) and same_bits(g_wide, again[1])
    strided = _grad_launch(c, fm, cuda, ldx_pad=3 if c["D"] % 8 else 4)
    assert same_bits(g_deep, strided[0]) and same_bits(g_wide, strided[1])


# ----------------------------------------------------------------------------- 4: ADAGRAD
def adagrad_expect(c, fm, lr):
    """float64 expectation and bounds for the rows of the batch: (uniq, acc', w', bound of
    acc', bound of w') for the deep table and the same five for the wide one."""
    from paddle_operator_amd.ops.ctr import ref_run_sums
    uniq, G, Gw = ref_run_sums(c["ids"], c["dX"].double(), c["dlogit"].double(), c["ssum"].double() if fm else None,
                               c["deep"].double())
    u2, n = run_lengths(c["ids"], c["rows"])
    assert torch.equal(uniq, u2)
    n = n.double()
    out = []
    for g, acc0, w0, cg in ((G, c["acc_deep"], c["deep"], (n + 2 if fm else n - 1)[:, None]),
                            (Gw, c["acc_wide"], c["wide"], n - 1)):
        acc = acc0[uniq].double() + g * g
        upd = lr * g / acc.sqrt()
        w = w0[uniq].double() - upd
        b_acc = torch.from_numpy(half_ulp32(acc.numpy())) + (2 * cg + 1) * U * g * g
        b_w = torch.from_numpy(half_ulp32(w.numpy())) + (2 * cg + 4) * U * upd.abs()
        out.append((acc, w, b_acc, b_w))
    return uniq, out


@pytest.mark.gpu
@pytest.mark.parametrize("fm", [False, True])
@pytest.mark.parametrize("name", PATTERNS)
def test_ctr_bwd_adagrad_within_rounding_count(cuda, name, fm):
    """Also: untouched rows of all four arrays keep their bits, and the rate is read from
    the device scalar at run time (two launches, two rates, one tensor)."""
    from paddle_operator_amd.ops.ctr import ADAGRAD, ctr_sparse_step
    c = random_case(name)
    lr_dev = torch.zeros(1, device=cuda)
    worst = 0.0
    for rate in (0.05, 0.125):
        lr_dev.fill_(rate)
        lr = float(lr_dev.item())  # the fp32 value the kernel reads
        deep, wide = c["deep"].to(cuda), c["wide"].to(cuda)
        acc_d, acc_w = c["acc_deep"].to(cuda), c["acc_wide"].to(cuda)
        ctr_sparse_step(c["ids"].to(cuda), c["dX"].to(cuda), c["dlogit"].to(cuda), c["ssum"].to(cuda) if fm else None,
                        (deep, wide), (acc_d, acc_w), lr_dev, ADAGRAD)
        uniq, exp = adagrad_expect(c, fm, lr)
        for (acc, w, b_acc, b_w), got_acc, got_w in zip(exp, (acc_d, acc_w), (deep, wide)):
            e_acc = (got_acc.cpu()[uniq].double() - acc).abs()
            e_w = (got_w.cpu()[uniq].double() - w).abs()
            worst = max(worst, float((e_acc / b_acc).max()), float((e_w / b_w).max()))
            assert (e_acc <= b_acc).all() and (e_w <= b_w).all()
        rest = torch.ones(c["rows"], dtype=torch.bool)
        rest[uniq] = False
        for got, before in ((deep, c["deep"]), (wide, c["wide"]), (acc_d, c["acc_deep"]), (acc_w, c["acc_wide"])):
            assert same_bits(got.cpu()[rest], before[rest])
    print(f"{name} fm={fm}: worst error / bound = {worst:.3f}")


@pytest.mark.gpu
def test_ctr_contract_refused_on_device(cuda):
    from paddle_operator_amd.ops.ctr import GRAD, ctr_lookup, ctr_sparse_step
    for D in (6, 68):
        ids = torch.zeros(2, 3, dtype=torch.int64, device=cuda)
        deep, wide = torch.zeros(4, D, device=cuda), torch.zeros(4, device=cuda)
        with pytest.raises((ValueError, RuntimeError)):
            ctr_lookup(ids, torch.zeros(2, 0, device=cuda), deep, wide, False)
        with pytest.raises((ValueError, RuntimeError)):
            ctr_sparse_step(ids, torch.zeros(2, 3 * D, device=cuda), torch.zeros(2, device=cuda), None, (deep, wide),
                            (torch.zeros_like(deep), torch.zeros_like(wide)), None, GRAD)


# ----------------------------------------------------------------------------- 5: model level
def dense_reference_step(model_sd, cfg, ids, dense, label, dtype, sparse_lr):
    """One step of models.wide_deep.WideDeep with autograd and the Adagrad rule applied to the
    dense table gradients (accumulators start at 0.1): (logits, loss, deep', wide') in ``dtype``."""
    import torch.nn.functional as F
    from paddle_operator_amd.models.wide_deep import WideDeep
    m = WideDeep(cfg).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in model_sd.items()})
    logit = m(ids, dense.to(dtype))
    loss = F.binary_cross_entropy_with_logits(logit, label.to(dtype))
    loss.backward()
    out = [logit.detach(), loss.detach()]
    for p in (m.deep_emb.weight, m.wide.weight):
        g = p.grad
        acc = torch.full_like(g, 0.1) + g * g
        out += [(p.detach() - sparse_lr * g / acc.sqrt())]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["wide_deep", "deepfm"])
def test_ctr_trainer_step_against_float64_model(cuda, model):
    """Logits, loss and the touched table rows of one CTRTrainer step at --tiny size against
    WideDeep in float64 on the CPU.  Yardstick: the same model in fp32 on the CPU; both are
    fp32 paths that differ in summation order, so the HIP path may have at most twice the
    yardstick's error (max over the quantity) plus one fp32 ulp at the value's magnitude."""
    from paddle_operator_amd.models.wide_deep import WideDeepConfig
    from paddle_operator_amd.workloads.ctr import TRAIN_STREAM, CTRTrainer
    cfg = WideDeepConfig(vocab_per_slot=1000, model=model)
    tr = CTRTrainer(cfg, 64, cuda, data_seed=3)
    sd = {k: v.clone() for k, v in tr.state_dict()["model"].items()}
    ids, dense, label = (t.cpu() for t in tr.draw(TRAIN_STREAM, 0))
    logit = tr.forward(ids.to(cuda), dense.to(cuda))[0].detach().cpu()
    loss = tr.step().cpu()
    uniq = torch.unique(ids)
    got = [logit, loss, tr.deep.cpu()[uniq], tr.wide.cpu()[uniq]]
    ref64 = dense_reference_step(sd, cfg, ids, dense, label, torch.float64, tr.sparse_lr)
    ref32 = dense_reference_step(sd, cfg, ids, dense, label, torch.float32, tr.sparse_lr)
    bad = []
    for name, g, r64, r32 in zip(("logits", "loss", "deep rows", "wide rows"), got, ref64, ref32):
        if name.endswith("rows"):
            r64, r32 = r64[uniq], r32[uniq]
        err = float((g.double() - r64).abs().max())
        yard = float((r32.double() - r64).abs().max())
        ulp = float(np.spacing(np.float32(r64.abs().max())))
        print(f"{model} {name}: hip err {err:.3e}, cpu fp32 err {yard:.3e}, ratio {err / max(yard, 1e-300):.2f}, "
              f"ulp {ulp:.3e}")
        if not err <= 2 * yard + ulp:
            bad.append((name, err, yard, ulp))
    assert not bad, bad


# ----------------------------------------------------------------------------- 6: launcher
def _launch(args, log, limit=240):
    env = dict(os.environ, PYTHONPATH=REPO, PDO_OPS="hip")
    for k in ("PADDLE_TRAINER_ID", "PADDLE_TRAINER_ENDPOINTS", "PADDLE_PSERVERS_IP_PORT_LIST", "TRAINING_ROLE"):
        env.pop(k, None)
    with open(log, "w") as f:
        rc = subprocess.run([sys.executable, "-m", "paddle_operator_amd.launch"] + args, env=env, cwd=REPO, stdout=f,
                            stderr=subprocess.STDOUT, timeout=limit).returncode
    assert rc == 0, open(log).read()[-3000:]


def _flat_state(st, prefix=""):
    out = {}
    for k, v in st.items():
        if isinstance(v, dict):
            out.update(_flat_state(v, f"{prefix}{k}."))
        elif torch.is_tensor(v):
            out[prefix + str(k)] = v
    return out


def assert_same_state(a, b):
    fa, fb = _flat_state(a), _flat_state(b)
    assert fa.keys() == fb.keys()
    diff = [k for k in fa if not torch.equal(fa[k], fb[k])]
    assert not diff, diff


@pytest.mark.gpu
def test_ctr_launcher_resume_is_bit_exact(cuda, tmp_path):
    """20 steps straight = 10 steps, checkpoint, 10 steps resumed, bit for bit: the sparse
    path is deterministic and the tower's kernels are the same in both runs.  The checkpoint
    loads into models.wide_deep.WideDeep."""
    from paddle_operator_amd.models.wide_deep import WideDeep, WideDeepConfig
    from paddle_operator_amd.utils import checkpoint as ckpt
    base = ["--workload", "wide_deep", "--tiny", "--log-every", "5"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _launch(base + ["--steps", "20", "--ckpt-dir", a], tmp_path / "a.log")
    _launch(base + ["--steps", "10", "--ckpt-dir", b], tmp_path / "b1.log")
    _launch(base + ["--steps", "20", "--ckpt-dir", b], tmp_path / "b2.log")
    assert "resumed from step 10" in open(tmp_path / "b2.log").read()
    sa, step_a = ckpt.load_latest(a)
    sb, step_b = ckpt.load_latest(b)
    assert step_a == step_b == 20
    assert_same_state(sa, sb)
    m = WideDeep(WideDeepConfig(vocab_per_slot=1000))
    m.load_state_dict(sa["model"])
    assert float(m.wide.weight.detach().abs().max()) > 0  # trained rows


# ----------------------------------------------------------------------------- 7: two ranks, one GPU
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, outdir, device, model):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from paddle_operator_amd.models.wide_deep import WideDeepConfig
    from paddle_operator_amd.workloads.ctr import CTRTrainer
    if device == "cuda":
        torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = CTRTrainer(WideDeepConfig(vocab_per_slot=1000, model=model), 64, torch.device(device))
    tr.sync_initial_weights()
    losses = [float(tr.step()) for _ in range(3)]
    sd = tr.state_dict()
    torch.save({"state": {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()}, "losses": losses},
               os.path.join(outdir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def spawn_ranks(fn, args, world, limit=240):
    """Start ``world`` processes and wait for them under a time limit; the first non-zero
    exit (or the limit) ends all of them and fails the test."""
    import torch.multiprocessing as mp
    ctx = mp.start_processes(fn, args=args, nprocs=world, start_method="spawn", join=False)
    end = time.time() + limit
    try:
        while not ctx.join(timeout=5):  # raises on a failed rank, after ending the others
            assert time.time() < end, "ranks ran past their time limit"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()


@pytest.mark.gpu
def test_ctr_two_ranks_one_gpu_replicas_identical(cuda, tmp_path):
    spawn_ranks(_rank_worker, (2, _port(), str(tmp_path), "cuda", "deepfm"), 2)
    r0, r1 = (torch.load(tmp_path / f"r{r}.pt", weights_only=True) for r in range(2))
    for k in ("deep_acc", "wide_acc"):
        assert same_bits(r0["state"][k], r1["state"][k]), k
    for k in ("deep_emb.weight", "wide.weight"):
        assert same_bits(r0["state"]["model"][k], r1["state"]["model"][k]), k
    assert float(r0["state"]["model"]["wide.weight"].abs().max()) > 0
