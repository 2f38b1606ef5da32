"""The DROP instantiations of the three flash-attention kernels (csrc/hip/attention.hip)
against the host mask reference ``ops.core.philox_attn_keep_mask``.

Exact tests: with Q = K = 0 every causal probability is P(q, k) = 1/(q + 1), and one-hot
V / dO / K columns make single mask elements visible in o, dV and dQ, so the mask each
kernel draws is recovered element by element over the whole causal triangle.  Numerics:
random inputs at p = 0.1 against an fp32 explicit-mask computation, with the framework's
bf16 form of the same computation as the yardstick.  Then the fused QKV node, repeat
calls, None specs, and one production step of the model against fp32 with the same masks.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D = 64
SEED = 0x9E3779B97F4A7C15  # both key words non-zero
SITE, STEP = 0x10000 + 3, 5
# (1, 128, 1): the single diagonal block; (2, 256, 2): off-diagonal tiles, batch / head indexing;
# (1, 512, 2): wraps the 3-slot Q / dO ring of dK/dV, both parities of the 64-key tile
SHAPES = [(1, 128, 1), (2, 256, 2), (1, 512, 2)]
THR8 = 77  # p ≈ 0.3: neither the kept nor the dropped elements are rare


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def _ops():
    from paddle_operator_amd import _native, ops
    _native.require_hip()
    return ops


def _kw(thr8=THR8):
    return dict(thr=thr8, seed=SEED, site=SITE, step=STEP)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _keep(B, S, H, dev, thr8=THR8):
    from paddle_operator_amd.ops.core import philox_attn_keep_mask
    return philox_attn_keep_mask(B, H, S, thr8, SEED, SITE, STEP).to(dev)  # [B, H, q, k]


def _tril(S, dev):
    return torch.ones(S, S, dtype=torch.bool, device=dev).tril()


def _onehot_window(S, base, dev):
    """[S, 64]: row r = e_{r − base} for base ≤ r < base + 64, else 0."""
    t = torch.zeros(S, D, device=dev)
    i = torch.arange(64, device=dev)
    t[base + i, i] = 1.0
    return t


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_forward_mask_recovery(cuda, B, S, H):
    """o[q, c] ≠ 0 ⇔ keep(q, base + c) for V = one-hot over the 64-key window at base."""
    m = _m()
    keep, tri = _keep(B, S, H, cuda), _tril(S, cuda)
    got = torch.zeros(B, H, S, S, dtype=torch.bool, device=cuda)
    for base in range(0, S, 64):
        qkv = torch.zeros(B, S, 3, H, D, device=cuda)
        qkv[:, :, 2] = _onehot_window(S, base, cuda)[None, :, None, :]
        qkv = qkv.to(BF16).view(B, S, 3 * H * D)
        o, lse = m.attn_fwd(qkv, H, **_kw())
        got[:, :, :, base:base + 64] = (o.view(B, S, H, D) != 0).permute(0, 2, 1, 3)
        # lse is that of the undropped softmax: the plain kernel's, bit for bit
        assert torch.equal(_bits(lse), _bits(m.attn_fwd(qkv, H)[1]))
    assert 0 < int((~keep & tri).sum()) and 0 < int((keep & tri).sum())
    bad = (got != keep) & tri
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:8].tolist())
    assert not bool((got & ~tri).any())  # above the diagonal: masked


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_dkdv_mask_recovery(cuda, B, S, H):
    """dV[k, c] ≠ 0 ⇔ keep(base + c, k) for dO = one-hot over the 64-query window at base."""
    m = _m()
    keep, tri = _keep(B, S, H, cuda), _tril(S, cuda)
    qkv = torch.zeros(B, S, 3 * H * D, device=cuda, dtype=BF16)
    o, lse = m.attn_fwd(qkv, H, **_kw())
    got = torch.zeros(B, H, S, S, dtype=torch.bool, device=cuda)
    for base in range(0, S, 64):
        do = _onehot_window(S, base, cuda)[None, :, None, :].expand(B, S, H, D).reshape(B, S, H * D).to(BF16)
        dqkv = m.attn_bwd(do.contiguous(), qkv, o, lse, H, **_kw())[0]
        dv = dqkv.view(B, S, 3, H, D)[:, :, 2]  # [B, k, H, c]
        got[:, :, base:base + 64, :] = (dv != 0).permute(0, 2, 3, 1)  # → [B, H, c (query), k]
    bad = (got != keep) & tri
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:8].tolist())
    assert not bool((got & ~tri).any())


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_dq_mask_recovery(cuda, B, S, H):
    """Q = 0, K = one-hot over the 64-key window at base, V[k] = e0, dO[q] = e0: dP = 1 and
    dQ[q, c] = ss/(q + 1) · (keep(q, base + c)·sd − delta_q), two values per row separated by
    ss·sd/(q + 1); each element is classified against their midpoint, taken from the host mask."""
    from paddle_operator_amd.ops.core import attn_dropout_spec
    m = _m()
    keep, tri = _keep(B, S, H, cuda), _tril(S, cuda)
    sd = attn_dropout_spec(THR8 / 256.0, SEED, SITE, STEP).scale
    ss = 1.0 / 8.0
    n1 = torch.arange(1, S + 1, device=cuda, dtype=torch.float64)  # q + 1
    delta = sd * (keep & tri).sum(-1).double() / n1  # [B, H, q] = o[q, 0]·dO[q, 0]
    mid = ss / n1 * (sd / 2 - delta)
    e0 = torch.zeros(D, device=cuda)
    e0[0] = 1.0
    do = e0.expand(B, S, H, D).reshape(B, S, H * D).to(BF16).contiguous()
    got = torch.zeros(B, H, S, S, dtype=torch.bool, device=cuda)
    for base in range(0, S, 64):
        qkv = torch.zeros(B, S, 3, H, D, device=cuda)
        qkv[:, :, 1] = _onehot_window(S, base, cuda)[None, :, None, :]
        qkv[:, :, 2] = e0
        qkv = qkv.to(BF16).view(B, S, 3 * H * D)
        o, lse = m.attn_fwd(qkv, H, **_kw())
        dq = m.attn_bwd(do, qkv, o, lse, H, **_kw())[0].view(B, S, 3, H, D)[:, :, 0]  # [B, q, H, c]
        got[:, :, :, base:base + 64] = dq.permute(0, 2, 1, 3).double() > mid[..., None]
    bad = (got != keep) & tri
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:8].tolist())


def test_mask_recovery_past_31_bit_slices(cuda):
    """S·3·H·64·2 B ≥ 2^31: the forward and dQ kernels leave their buffer-load variants for the
    pointer-staging ones, whose DROP instantiations must draw the same mask.  S = 128 and
    H = 43691 (a 2 GiB qkv); the forward and dQ recoveries above on a few heads, first to last.
    Memory: one qkv (2 GiB), o and dO (0.7 GiB each), dqkv (2 GiB) and the backward's workspace
    are alive at once, about 6 GiB at the peak, freed before the next window; about 2 s."""
    from paddle_operator_amd.ops.core import attn_dropout_spec, philox_attn_keep_mask
    m = _m()
    S, H = 128, 43691
    assert S * 3 * H * D * 2 >= 1 << 31
    heads = [0, 1, H // 2, H - 1]
    keep = torch.stack([philox_attn_keep_mask(1, 1, S, THR8, SEED, SITE, STEP, bh0=h)[0, 0] for h in heads]).to(cuda)
    tri = _tril(S, cuda)
    sd, ss = attn_dropout_spec(THR8 / 256.0, SEED, SITE, STEP).scale, 1.0 / 8.0
    n1 = torch.arange(1, S + 1, device=cuda, dtype=torch.float64)
    mid = ss / n1 * (sd / 2 - sd * (keep & tri).sum(-1).double() / n1)  # [head, q]
    e0 = torch.zeros(D, device=cuda, dtype=BF16)
    e0[0] = 1.0
    do = e0.expand(1, S, H, D).reshape(1, S, H * D).contiguous()
    got_f = torch.zeros(len(heads), S, S, dtype=torch.bool, device=cuda)
    got_q = torch.zeros_like(got_f)
    for base in range(0, S, 64):
        win = _onehot_window(S, base, cuda).to(BF16)[:, None, :]
        qkv = torch.zeros(1, S, 3, H, D, device=cuda, dtype=BF16)
        qkv[0, :, 2] = win
        o, _ = m.attn_fwd(qkv.view(1, S, 3 * H * D), H, **_kw())
        got_f[:, :, base:base + 64] = (o.view(S, H, D)[:, heads] != 0).permute(1, 0, 2)
        qkv[0, :, 1] = win
        qkv[0, :, 2] = e0
        qkv = qkv.view(1, S, 3 * H * D)
        o, lse = m.attn_fwd(qkv, H, **_kw())
        dq = m.attn_bwd(do, qkv, o, lse, H, **_kw())[0].view(S, 3, H, D)[:, 0][:, heads]  # [q, head, c]
        got_q[:, :, base:base + 64] = dq.permute(1, 0, 2).double() > mid[..., None]
        del qkv, o, lse, dq
    for got in (got_f, got_q):
        bad = (got != keep) & tri
        assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:8].tolist())


# ---------------------------------------------------------------------------------------------
# numerics at p = 0.1
# ---------------------------------------------------------------------------------------------
_NUM = {}


def _numerics(cuda, B, S, H):
    """fp32 and framework-bf16 explicit-mask results and the HIP ones, computed once per shape."""
    key = (B, S, H)
    if key in _NUM:
        return _NUM[key]
    ops = _ops()
    from paddle_operator_amd.ops.core import attn_dropout_spec, philox_attn_keep_mask, ref_attention
    g = torch.Generator(device=cuda).manual_seed(100 + S)
    qkv = torch.randn(B, S, 3 * H * D, device=cuda, generator=g).to(BF16)
    do = torch.randn(B, S, H * D, device=cuda, generator=g).to(BF16)
    spec = attn_dropout_spec(0.1, SEED, SITE, STEP)
    keep = philox_attn_keep_mask(B, H, S, spec.thr, SEED, SITE, STEP).to(cuda)

    def explicit(dtype):
        x = qkv.to(dtype).requires_grad_()
        q, k, v = x.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
        o = ref_attention(q, k, v, causal=True, keep=keep, scale=spec.scale, math_dtype=dtype)
        o = o.transpose(1, 2).reshape(B, S, H * D)
        o.backward(do.to(dtype))
        gq = x.grad.view(B, S, 3, H * D)
        return [t.detach().float() for t in (o, gq[:, :, 0], gq[:, :, 1], gq[:, :, 2])]

    x = qkv.clone().requires_grad_()
    o = ops.attention(x, H, drop=spec)
    o.backward(do)
    gq = x.grad.view(B, S, 3, H * D)
    hip = [t.detach().float() for t in (o, gq[:, :, 0], gq[:, :, 1], gq[:, :, 2])]
    _NUM[key] = (hip, explicit(torch.float32), explicit(BF16))
    return _NUM[key]


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_numerics_vs_fp32_same_mask(cuda, B, S, H):
    """o, dq, dk, dv: HIP relative error ≤ 1.5 × the framework-bf16 error of the same
    explicit-mask computation + 0.005, whole tensor and per 128-row block."""
    hip, ref, fw = _numerics(cuda, B, S, H)
    bad = []
    for name, h, r, f in zip(("o", "dq", "dk", "dv"), hip, ref, fw):
        eh, ef = _rel(h, r), _rel(f, r)
        worst = eh / (1.5 * ef + 0.005)
        if not eh <= 1.5 * ef + 0.005:
            bad.append((name, "all", eh, ef))
        for b in range(B):
            for blk in range(S // 128):
                sl = (b, slice(128 * blk, 128 * blk + 128))
                ehb, efb = _rel(h[sl], r[sl]), _rel(f[sl], r[sl])
                worst = max(worst, ehb / (1.5 * efb + 0.005))
                if not ehb <= 1.5 * efb + 0.005:
                    bad.append((name, (b, blk), ehb, efb))
        print(f"attn dropout numerics B{B} S{S} H{H} {name}: hip {eh:.3e} framework-bf16 {ef:.3e}; "
              f"max err / (1.5·framework + 0.005) over blocks = {worst:.3f}")
    assert not bad, bad


def test_qkv_fused_path_with_dropout(cuda):
    """_QKVAttnFn with a spec (bias gradient from the DROP kernels' column partials) == the
    separate linear + attention nodes with the same spec; the bar of
    test_qkv_attention_fused_bias_grad (max-abs error relative to the max, < 1e-2)."""
    ops = _ops()
    from paddle_operator_amd.ops.core import attn_dropout_spec
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))  # noqa: E731
    B, S, H, C = 2, 256, 4, 256
    g = torch.Generator(device=cuda).manual_seed(21)
    base = [torch.randn(B, S, C, device=cuda, generator=g).bfloat16(),
            (0.05 * torch.randn(3 * C, C, device=cuda, generator=g)).bfloat16(),
            (0.1 * torch.randn(3 * C, device=cuda, generator=g)).bfloat16()]
    do = torch.randn(B, S, C, device=cuda, generator=g).bfloat16()
    spec = attn_dropout_spec(0.1, SEED, SITE, STEP)
    outs, grads = [], []
    for fused in (True, False):
        ops._QKV_FUSED[0] = fused
        try:
            ts = [t.clone().requires_grad_() for t in base]
            o = ops.qkv_attention(ts[0], ts[1], ts[2], H, drop=spec)
            o.backward(do)
        finally:
            ops._QKV_FUSED[0] = True
        outs.append(o.detach().float())
        grads.append([t.grad.float() for t in ts])
    assert rel(outs[0], outs[1]) < 1e-2
    for a, b, name in zip(grads[0], grads[1], ("dh", "dw", "db")):
        assert rel(a, b) < 1e-2, name
    # and the dropout is really on in both
    ts = [t.clone() for t in base]
    assert rel(ops.qkv_attention(ts[0], ts[1], ts[2], H).float(), outs[0]) > 5e-2


def test_repeat_calls_and_none_specs(cuda):
    ops = _ops()
    from paddle_operator_amd.ops.core import Dropout, attn_dropout_spec
    B, S, H = 2, 256, 2
    g = torch.Generator(device=cuda).manual_seed(8)
    qkv = torch.randn(B, S, 3 * H * D, device=cuda, generator=g).to(BF16)
    do = torch.randn(B, S, H * D, device=cuda, generator=g).to(BF16)

    def run(**kw):
        x = qkv.clone().requires_grad_()
        o = ops.attention(x, H, **kw)
        o.backward(do)
        return o.detach(), x.grad

    spec = attn_dropout_spec(0.1, SEED, SITE, STEP)
    (o1, g1), (o2, g2) = run(drop=spec), run(drop=spec)
    assert torch.equal(_bits(o1), _bits(o2)) and torch.equal(_bits(g1), _bits(g2))
    o0, g0 = run()
    assert not torch.equal(_bits(o1), _bits(o0))
    for none in (None, Dropout(0, 1.0, SEED, SITE, STEP), attn_dropout_spec(0.0, SEED, SITE, STEP)):
        on, gn = run(drop=none)
        assert torch.equal(_bits(on), _bits(o0)) and torch.equal(_bits(gn), _bits(g0))
    # the extension itself: thr = 0 is the plain kernel, thr > 255 is rejected
    m = _m()
    assert torch.equal(_bits(m.attn_fwd(qkv, H, thr=0, seed=SEED, site=SITE, step=STEP)[0]), _bits(m.attn_fwd(qkv, H)[0]))
    with pytest.raises(RuntimeError):
        m.attn_fwd(qkv, H, thr=256, seed=SEED, site=SITE, step=STEP)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# model level: gpt2-smoke, B = 2, S = 256, every dropout at 0.1
# ---------------------------------------------------------------------------------------------
MB, MS = 2, 256


def _mrel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))


def _smoke_cfg(p=0.1, attn=0.1):
    from paddle_operator_amd.models.gpt2 import GPT2Config
    cfg = GPT2Config.named("gpt2-smoke")
    cfg.n_positions = max(cfg.n_positions, MS)
    cfg.embd_pdrop = cfg.resid_pdrop = p
    cfg.attn_pdrop = attn
    return cfg


@pytest.fixture(scope="module")
def trained(cuda):
    """One production step (GPT2Trainer.step), teacher-forced: the weights before the step,
    the batch, the loss and the arena gradients."""
    from paddle_operator_amd.train import GPT2Trainer
    tr = GPT2Trainer(_smoke_cfg(), MB, MS, cuda, dropout_seed=7)
    tr.drop_step = 3
    x, y = tr.batch()
    master0 = tr.opt.master.clone()
    loss = float(tr.step(x, y).detach())
    flat = tr.flat
    view = lambda buf, s: buf[s.offset:s.offset + s.numel].view(s.shape)  # noqa: E731
    grads = {s.name: (view(flat.param_grads, s).float() * tr.ddp.grad_scale).clone() for s in flat.slots}
    torch.cuda.synchronize()
    return dict(tr=tr, x=x, y=y, master0=master0, loss=loss, grads=grads, view=view, raw=flat.param_grads.clone())


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
    """Every parameter gradient of the HIP step within 1.5 × the framework-bf16 error + 0.005 of
    the same masked model (fp32 on the CPU; the framework in bf16 through PDO_OPS=torch), both
    drawing the kernels' masks on the host, attention masks included; |loss − loss_fp32| < 1e-2."""
    from paddle_operator_amd.models.gpt2 import GPT2
    tr, x, y = trained["tr"], trained["x"], trained["y"]
    cfg = _smoke_cfg()
    ref = GPT2(cfg)  # fp32, CPU
    with torch.device(cuda):
        fw = GPT2(cfg).bfloat16()
    loss_r, g_r = _ref_grads(ref, tr, trained["master0"], trained["view"], x, y, 3)
    loss_f, g_f = _ref_grads(fw, tr, trained["master0"], trained["view"], x, y, 3)
    errs = {n: (_mrel(trained["grads"][n].cpu(), g_r[n]), _mrel(g_f[n], g_r[n])) for n in g_r}
    ratio = max(eh / (1.5 * ef + 0.005) for eh, ef in errs.values())
    worst = max(errs, key=lambda n: errs[n][0] / (1.5 * errs[n][1] + 0.005))
    print(f"attention-dropout model anchor: loss hip {trained['loss']:.5f} fp32 {loss_r:.5f} framework-bf16 "
          f"{loss_f:.5f}; max err / (1.5·framework + 0.005) = {ratio:.3f} at {worst} {errs[worst]}")
    assert abs(trained["loss"] - loss_r) < 1e-2, (trained["loss"], loss_r, loss_f)
    bad = {n: (round(eh, 4), round(ef, 4)) for n, (eh, ef) in errs.items() if not eh <= 1.5 * ef + 0.005}
    assert not bad, bad


def test_model_repeatable(cuda, trained):
    """A second trainer with the same seed and step: bit-identical loss and arena gradients."""
    from paddle_operator_amd.train import GPT2Trainer
    tr2 = GPT2Trainer(_smoke_cfg(), MB, MS, cuda, dropout_seed=7)
    tr2.drop_step = 3
    loss = float(tr2.step(trained["x"], trained["y"]).detach())
    assert loss == trained["loss"]
    assert torch.equal(_bits(tr2.flat.param_grads), _bits(trained["raw"]))
    # the attention masks take part: with attention dropout alone switched off the step differs
    tr3 = GPT2Trainer(_smoke_cfg(0.1, 0.0), MB, MS, cuda, dropout_seed=7)
    tr3.drop_step = 3
    assert float(tr3.step(trained["x"], trained["y"]).detach()) != trained["loss"]
