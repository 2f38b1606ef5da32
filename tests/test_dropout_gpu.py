"""The DROP instantiations of the LayerNorm and embedding kernels against the
host mask reference (``ops.core.philox_keep_mask``), called straight through the
extension, and the GPT-2 model / trainer with dropout on.

Exact tests: integer-valued bf16 inputs in [−8, 8] and p = 0.5 / 0.75 (scale 2 /
4, powers of two), so every product and sum of the dropout path is exact in fp32
whether or not the compiler contracts it into an FMA, and the dropped residual
r' = bf16(drop(r + rbias)) is exactly representable: the DROP kernel must then
agree bit for bit with the plain kernel fed r'.
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
U = 2.0 ** -24
EPS = 1e-5
SEED = 0x9E3779B97F4A7C15  # both key words non-zero
SHAPES = [(7, 256), (37, 776), (64, 1024), (5, 2048)]
OFFSETS = [0, (1 << 32) - 3]  # the second: the carry into the counter's second word falls inside the tensor
PS = [(0.5, 2.0), (0.75, 4.0)]


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def _gen(dev, seed=0):
    return torch.Generator(device=dev).manual_seed(seed)


def _ints(shape, dev, gen, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, device=dev, generator=gen).to(BF16)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _keep(shape, p, site, step, offset, dev):
    from paddle_operator_amd.ops.core import dropout_thr, philox_keep_mask
    return philox_keep_mask(shape, dropout_thr(p), SEED, site, step, offset).to(dev)


def _kw(p, site, step, offset):
    from paddle_operator_amd.ops.core import dropout_thr
    return dict(thr=dropout_thr(p), seed=SEED, site=site, step=step, offset=offset)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("p,scale", PS)
@pytest.mark.parametrize("N,C", SHAPES)
def test_add_layernorm_fwd_drop_exact(cuda, N, C, p, scale, offset):
    m, g = _m(), _gen(cuda, 1)
    x, r = _ints((N, C), cuda, g), _ints((N, C), cuda, g)
    rb, w, b = _ints((C,), cuda, g), _ints((C,), cuda, g, -2, 2), _ints((C,), cuda, g)
    keep = _keep((N, C), p, 3, 5, offset, cuda)
    assert 0 < int(keep.sum()) < keep.numel()
    for rbias in (rb, None):
        h, y, mean, rstd = m.add_layernorm_fwd(x, r, w, b, EPS, rbias, **_kw(p, 3, 5, offset))
        t = r.float() if rbias is None else r.float() + rbias.float()
        dropped = torch.where(keep, t * scale, torch.zeros((), device=cuda))  # exact: integers ≤ 64
        rp = dropped.to(BF16)
        assert torch.equal(rp.float(), dropped)
        assert same_bits(h, (x.float() + dropped).to(BF16))
        h2, y2, mean2, rstd2 = m.add_layernorm_fwd(x, rp, w, b, EPS)  # the plain kernel on r'
        assert same_bits(h, h2) and same_bits(y, y2) and same_bits(mean, mean2) and same_bits(rstd, rstd2)
    # thr = 0 dispatches to the plain kernel: nothing dropped
    h0 = m.add_layernorm_fwd(x, r, w, b, EPS, rb, thr=0, seed=SEED, site=3, step=5, offset=offset)[0]
    assert same_bits(h0, m.add_layernorm_fwd(x, r, w, b, EPS, rb)[0])


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("p,scale", PS)
@pytest.mark.parametrize("N,C", SHAPES)
def test_embed_fwd_drop_exact(cuda, N, C, p, scale, offset):
    m, g = _m(), _gen(cuda, 2)
    B, S = (4, N // 4) if N % 4 == 0 else (1, N)
    V = 50
    idx = torch.randint(0, V, (B, S), device=cuda, generator=g)
    wte, wpe = _ints((V, C), cuda, g), _ints((S + 3, C), cuda, g)
    keep = _keep((B, S, C), p, 0, 9, offset, cuda)
    y = m.embed_fwd(idx, wte, wpe, **_kw(p, 0, 9, offset))
    e = wte.float()[idx] + wpe.float()[:S].unsqueeze(0)
    want = torch.where(keep, e * scale, torch.zeros((), device=cuda)).to(BF16)
    assert same_bits(y, want)
    assert same_bits(m.embed_fwd(idx, wte, wpe, thr=0, seed=SEED), m.embed_fwd(idx, wte, wpe))


@pytest.mark.parametrize("p,scale", PS)
@pytest.mark.parametrize("N,C", SHAPES)
def test_layernorm_bwd_drop_exact(cuda, N, C, p, scale):
    m, g = _m(), _gen(cuda, 3)
    h, dy, dres = _ints((N, C), cuda, g), _ints((N, C), cuda, g), _ints((N, C), cuda, g)
    w, b = _ints((C,), cuda, g, -2, 2), _ints((C,), cuda, g)
    _, mean, rstd = m.layernorm_fwd(h, w, b, EPS)
    keep = _keep((N, C), p, 4, 2, 0, cuda)
    zero = torch.zeros((), device=cuda)
    for rbias in (False, True):
        plain = m.layernorm_bwd_add(dy, h, w, mean, rstd, dres, rbias)
        outs = m.layernorm_bwd_add(dy, h, w, mean, rstd, dres, rbias, **_kw(p, 4, 2, 0))
        assert len(outs) == len(plain) + 1
        dx, dw, db, ddrop = outs[0], outs[1], outs[2], outs[-1]
        # the residual stream's gradient and dgamma / dbeta: the plain kernel's, bit for bit
        assert same_bits(dx, plain[0]) and same_bits(dw, plain[1]) and same_bits(db, plain[2])
        want = torch.where(keep, dx.float() * scale, zero).to(BF16)  # +0 where dropped
        assert same_bits(ddrop, want)
        if rbias:
            # drbias = colsum of the masked, scaled gradient against the float64 column sum of
            # float(ddrop): 2^-9 relative per term (one bf16 rounding) + N fp32 accumulation
            # roundings of at most U·Σ|t| each; the output itself is bf16, so it must lie between
            # the roundings of the interval's ends.  (The kernel sums the terms as stored, after
            # their bf16 rounding, so only the accumulation roundings are actually spent.)
            t = ddrop.double()
            s, a = t.sum(0), t.abs().sum(0)
            bound = 2.0 ** -9 * a + N * U * a
            lo, hi = (s - bound).to(BF16).double(), (s + bound).to(BF16).double()
            drb = outs[3].double()
            print(f"drbias N={N} C={C} p={p}: max |drbias - sum| / bound, the output's own bf16 rounding included: "
                  f"{float(((drb - s).abs() / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool(((drb >= lo) & (drb <= hi)).all())
        # arena form (grads accumulate in place) without the dx store
        gd = [torch.zeros(C, device=cuda, dtype=BF16) for _ in range(3 if rbias else 2)]
        o2 = m.layernorm_bwd_add(dy, h, w, mean, rstd, dres, rbias, grads=gd, want_dx=False, **_kw(p, 4, 2, 0))
        assert len(o2) == 2 and o2[0].numel() == 0 and same_bits(o2[1], ddrop)
        assert same_bits(gd[0], dw) and same_bits(gd[1], db)
        if rbias:
            assert same_bits(gd[2], outs[3])


def test_drop_p01_random_inputs(cuda):
    """p = 0.1 (scale not a power of two), normal inputs, (37, 776): h and ddrop within 2^-8
    relative of float64 per element (one bf16 rounding plus fp32 slack), zeros exactly where
    the reference drops."""
    from paddle_operator_amd.ops.core import dropout_spec
    m, g = _m(), _gen(cuda, 4)
    N, C, p = 37, 776, 0.1
    rnd = lambda *s: torch.randn(*s, device=cuda, generator=g).to(BF16)  # noqa: E731
    x, r, rb, w, b = rnd(N, C), rnd(N, C), rnd(C), rnd(C), rnd(C)
    scale = dropout_spec(p, SEED, 1, 1).scale  # the fp32 value the kernel receives
    keep = _keep((N, C), p, 1, 1, 0, cuda)
    h, y, mean, rstd = m.add_layernorm_fwd(x, r, w, b, EPS, rb, **_kw(p, 1, 1, 0))
    t = (r.double() + rb.double()) * scale
    h64 = x.double() + torch.where(keep, t, torch.zeros((), device=cuda, dtype=torch.float64))
    rel = (h.double() - h64).abs() / h64.abs().clamp_min(1e-300)
    print(f"p=0.1 forward: max rel err of h {float(rel.max()):.3e} (bound {2.0 ** -8:.3e})")
    assert float(rel.max()) <= 2.0 ** -8
    assert same_bits(h[~keep], x[~keep])  # dropped: the residual stream passes through untouched
    dy, dres = rnd(N, C), rnd(N, C)
    plain = m.layernorm_bwd_add(dy, h, w, mean, rstd, dres, True)
    outs = m.layernorm_bwd_add(dy, h, w, mean, rstd, dres, True, **_kw(p, 1, 1, 0))
    dx, ddrop = outs[0], outs[-1]
    assert same_bits(dx, plain[0])
    # float64 gradient of the residual stream from the textbook formula, then mask · scale
    xh = (h.double() - mean.double()[:, None]) * rstd.double()[:, None]
    gg = dy.double() * w.double()
    o64 = (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) * rstd.double()[:, None] \
        + dres.double()
    d64 = torch.where(keep, o64 * scale, torch.zeros((), device=cuda, dtype=torch.float64))
    assert bool((ddrop[~keep].float() == 0).all()) and bool((_bits(ddrop)[~keep] == 0).all())
    rel = ((ddrop.double() - d64).abs() / d64.abs().clamp_min(1e-300))[keep]
    print(f"p=0.1 backward: max rel err of ddrop {float(rel.max()):.3e} (bound {2.0 ** -8:.3e})")
    assert float(rel.max()) <= 2.0 ** -8


def test_rejections(cuda):
    m, g = _m(), _gen(cuda, 5)
    N, C = 4, 64
    x, r, w, b, rb = (_ints(s, cuda, g) for s in ((N, C), (N, C), (C,), (C,), (C,)))
    _, mean, rstd = m.layernorm_fwd(x, w, b, EPS)
    ok = dict(seed=SEED, site=0, step=0, offset=0)
    with pytest.raises(RuntimeError):
        m.add_layernorm_fwd(x, r, w, b, EPS, rb, thr=65536, **ok)
    with pytest.raises(RuntimeError):
        m.add_layernorm_fwd(x, r, w, b, EPS, rb, thr=-1, **ok)
    with pytest.raises(RuntimeError):
        m.add_layernorm_fwd(x, None, w, b, EPS, rb, thr=100, **ok)  # rbias without r
    with pytest.raises(RuntimeError):
        m.add_layernorm_fwd(x, None, w, b, EPS, rb)
    with pytest.raises(RuntimeError):
        m.layernorm_bwd_add(x, x, w, mean, rstd, r, True, thr=65536, **ok)
    with pytest.raises(RuntimeError):
        m.layernorm_bwd_add(x, x, w, mean, rstd, r, True, want_dx=False)  # dx skipped only with dropout
    C2 = 68  # C % 8 != 0
    x2, w2 = _ints((N, C2), cuda, g), _ints((C2,), cuda, g)
    with pytest.raises(RuntimeError):
        m.add_layernorm_fwd(x2, x2, w2, w2, EPS, None, thr=100, **ok)
    with pytest.raises(RuntimeError):
        m.layernorm_bwd_add(x2, x2, w2, mean, rstd, x2, False, thr=100, **ok)
    idx = torch.zeros(1, N, dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError):
        m.embed_fwd(idx, x2, x2, thr=100, **ok)
    with pytest.raises(RuntimeError):
        m.embed_fwd(idx, x, x, thr=65536, **ok)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# model level: gpt2-smoke at the batch and sequence of tests/test_trainer_gpu.py
# ---------------------------------------------------------------------------------------------
B, S = 8, 1024


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))


def _smoke_cfg(p=0.0, attn=0.0):
    from paddle_operator_amd.models.gpt2 import GPT2Config
    cfg = GPT2Config.named("gpt2-smoke")
    cfg.n_positions = S  # gpt2-smoke's table holds 512 positions; the yardstick's sequence is 1024
    cfg.embd_pdrop = cfg.resid_pdrop = p
    cfg.attn_pdrop = attn
    return cfg


@pytest.fixture(scope="module")
def trained(cuda):
    """One production step (GPT2Trainer.step) of gpt2-smoke with p = 0.1, teacher-forced:
    the weights before the step, the batch, the loss and the arena gradients."""
    from paddle_operator_amd.train import GPT2Trainer
    tr = GPT2Trainer(_smoke_cfg(0.1), B, S, cuda, dropout_seed=7)
    tr.drop_step = 3
    x, y = tr.batch()
    master0 = tr.opt.master.clone()
    loss = float(tr.step(x, y).detach())
    flat = tr.flat
    view = lambda buf, s: buf[s.offset:s.offset + s.numel].view(s.shape)  # noqa: E731
    grads = {s.name: (view(flat.param_grads, s).float() * tr.ddp.grad_scale).clone() for s in flat.slots}
    torch.cuda.synchronize()
    return dict(tr=tr, x=x, y=y, master0=master0, loss=loss, grads=grads, view=view,
                raw=flat.param_grads.clone())


def _ref_grads(model, tr, master0, view, x, y, step):
    params = dict(model.named_parameters())
    with torch.no_grad():
        for s in tr.flat.slots:
            params[s.name].copy_(view(master0, s))
    model.train()
    model.drop_seed, model.drop_step = tr.model.drop_seed, step
    model.zero_grad(set_to_none=True)
    dev = next(model.parameters()).device
    old = os.environ.get("PDO_OPS")
    os.environ["PDO_OPS"] = "torch"
    try:
        loss = model(x.to(dev), y.to(dev))
        loss.backward()
    finally:
        if old is None:
            os.environ.pop("PDO_OPS")
        else:
            os.environ["PDO_OPS"] = old
    return float(loss.detach()), {n: p.grad.float().cpu() for n, p in params.items()}


def test_model_gradients_vs_fp32_same_masks(cuda, trained):
    """Every parameter gradient of the HIP step within 1.5× the framework-bf16 error (+ 0.005,
    the yardstick of tests/test_trainer_gpu.py) of the same masked model: fp32 on the CPU and
    the framework in bf16 (torch ops, PDO_OPS=torch) both draw the kernels' masks on the host."""
    from paddle_operator_amd.models.gpt2 import GPT2
    tr, x, y = trained["tr"], trained["x"], trained["y"]
    cfg = _smoke_cfg(0.1)
    ref = GPT2(cfg)  # fp32, CPU
    with torch.device(cuda):
        fw = GPT2(cfg).bfloat16()
    loss_r, g_r = _ref_grads(ref, tr, trained["master0"], trained["view"], x, y, 3)
    loss_f, g_f = _ref_grads(fw, tr, trained["master0"], trained["view"], x, y, 3)
    errs = {n: (_rel(trained["grads"][n].cpu(), g_r[n]), _rel(g_f[n], g_r[n])) for n in g_r}
    ratio = max(eh / (1.5 * ef + 0.005) for eh, ef in errs.values())
    worst = max(errs, key=lambda n: errs[n][0] / (1.5 * errs[n][1] + 0.005))
    print(f"dropout model anchor: loss hip {trained['loss']:.5f} fp32 {loss_r:.5f} framework-bf16 {loss_f:.5f}; "
          f"max err / (1.5·framework + 0.005) = {ratio:.3f} at {worst} {errs[worst]}")
    d = os.environ.get("PDO_TEST_DUMP_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "gpt2_dropout_anchor.json"), "w") as f:
            json.dump({"loss": [trained["loss"], loss_r, loss_f], "max_ratio": ratio, "grad_errs": errs}, f, indent=0)
    # a different mask would move the loss by far more than the bf16 error
    assert abs(trained["loss"] - loss_r) < 1e-2, (trained["loss"], loss_r, loss_f)
    bad = {n: (round(eh, 4), round(ef, 4)) for n, (eh, ef) in errs.items() if not eh <= 1.5 * ef + 0.005}
    assert not bad, bad


def test_model_repeatable(cuda, trained):
    """The same (seed, step), weights and batch: bit-identical loss and gradients."""
    from paddle_operator_amd.train import GPT2Trainer
    tr2 = GPT2Trainer(_smoke_cfg(0.1), B, S, cuda, dropout_seed=7)
    tr2.drop_step = 3
    loss = float(tr2.step(trained["x"], trained["y"]).detach())
    assert loss == trained["loss"]
    assert torch.equal(_bits(tr2.flat.param_grads), _bits(trained["raw"]))
    tr3 = GPT2Trainer(_smoke_cfg(0.1), B, S, cuda, dropout_seed=7)
    tr3.drop_step = 9  # another step number draws other masks
    assert float(tr3.step(trained["x"], trained["y"]).detach()) != trained["loss"]


def test_model_eval_is_the_p0_model(cuda, trained):
    from paddle_operator_amd.models.gpt2 import GPT2
    m1 = trained["tr"].model
    with torch.device(cuda):
        m0 = GPT2(_smoke_cfg(0.0)).bfloat16()
    m0.load_state_dict(m1.state_dict())
    x, y = trained["x"], trained["y"]
    with torch.no_grad():
        try:
            l1 = m1.eval()(x, y)
        finally:
            m1.train()
        l0 = m0.eval()(x, y)
        lt = m0.train()(x, y)  # p = 0 in training: the dropout-free step
        ld = m1(x, y)
    assert same_bits(l1, l0) and same_bits(lt, l0)
    assert not same_bits(ld, l0)


def test_attention_dropout(cuda):
    from paddle_operator_amd.models.gpt2 import GPT2
    with torch.device(cuda):
        m1 = GPT2(_smoke_cfg(0.0, 0.1)).bfloat16()
        m0 = GPT2(_smoke_cfg(0.0)).bfloat16()
    m0.load_state_dict(m1.state_dict())
    g = _gen(cuda, 6)
    idx = torch.randint(0, m1.cfg.vocab_size, (2, 129), device=cuda, generator=g)
    x, y = idx[:, :-1].contiguous(), idx[:, 1:].contiguous()
    loss = m1(x, y)
    loss.backward()
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m1.parameters())
    with torch.no_grad():
        assert same_bits(m1.eval()(x, y), m0.eval()(x, y))
