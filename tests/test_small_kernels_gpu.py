"""Exact and fp64 checks of the small kernels every training step runs.

optim.hip, reduce.hip, bucket.hip, xent.hip, the batched transpose and the
fp32 → bf16 cast, called straight through the extension.  Where the arithmetic
allows it the inputs are integer-valued bf16 of small magnitude: fp32 sums of
integers below 2^24 are exact and the single final bf16 round-to-nearest-even
is fixed, so the output must equal the float64 reference bit for bit and one
dropped, doubled or misplaced element fails the test.  The optimizer and the
cross-entropy kernels are bounded against float64 references by counted fp32
roundings (u = 2^-24).

Every tensor handed to a kernel is a fresh allocation or a slice that starts at
a multiple of 1024 elements; every rejection is raised by the binding before
any launch.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF16 = torch.bfloat16


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def f32(x):
    """x rounded to float32, as a Python float: what a kernel receives for a scalar argument."""
    return float(np.float32(x))


def _gen(dev, seed=0):
    return torch.Generator(device=dev).manual_seed(seed)


def _ints(shape, lo, hi, dev, gen, dtype=BF16):
    return torch.randint(lo, hi + 1, shape, device=dev, generator=gen).to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _worst(err, bound):
    """max err / bound (a bound of 0 admits only err = 0)."""
    return float((err / bound.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------
# references (float64, plain textbook formulas; validated on the CPU in test_small_kernels_cpu.py)
# ---------------------------------------------------------------------------------------------
def clip_coef(normsq, clip, grad_scale):
    """grad_scale · min(1, clip / (‖g‖ + 1e-6)); clip ≤ 0 disables clipping (normsq is not read)."""
    if clip <= 0:
        return grad_scale
    return grad_scale * min(1.0, clip / (math.sqrt(normsq) + 1e-6))


def adamw_ref(w, m, v, g, dec, c, lr, b1, b2, eps, wd, bc1, bc2):
    """One decoupled-weight-decay Adam step in the tensors' own precision (float64 here).

    g is the raw gradient and c the coefficient applied to it beforehand (grad_scale · clip);
    dec is 1 where the weight decays and 0 where it does not; bc1 = 1 − b1^t, bc2 = 1 − b2^t.
    Returns (w, m, v, upd) with upd the bias-corrected direction m̂ / (√v̂ + eps)."""
    gg = c * g
    m = b1 * m + (1.0 - b1) * gg
    v = b2 * v + (1.0 - b2) * gg * gg
    upd = (m / bc1) / (v.sqrt() / math.sqrt(bc2) + eps)
    w = w * (1.0 - lr * wd * dec) - lr * upd
    return w, m, v, upd


def sgd_ref(w, buf, g, dec, lr, mom, wd, grad_scale):
    """Momentum SGD with L2 decay folded into the gradient: returns (w, buf)."""
    buf = mom * buf + (g * grad_scale + wd * dec * w)
    return w - lr * buf, buf


def xent_ref(logits, tgt, V, dloss=1.0):
    """float64 cross entropy over the first V columns, mean over targets in [0, V).

    Returns (loss, lse [N], dlogits [N, Vp], count)."""
    x = logits[:, :V].double()
    N, Vp = logits.shape
    lse = torch.logsumexp(x, dim=1)
    valid = (tgt >= 0) & (tgt < V)
    cnt = int(valid.sum())
    d = torch.zeros(N, Vp, dtype=torch.float64, device=logits.device)
    if cnt == 0:
        return 0.0, lse, d, 0
    rows = valid.nonzero().flatten()
    t = tgt[rows]
    loss = float((lse[rows] - x[rows, t]).sum() / cnt)
    p = torch.exp(x[rows] - lse[rows, None])
    p[torch.arange(len(rows), device=p.device), t] -= 1.0
    d[rows, :V] = p * (dloss / cnt)
    return loss, lse, d, cnt


# ---------------------------------------------------------------------------------------------
# 0. flatten_scale / unflatten: sentinels around every tensor, first offset > 0
# ---------------------------------------------------------------------------------------------
SENT = 1984.0  # exact in bf16, far outside the data


def _bucket_layout():
    """106 tensors: first offset 24, odd sizes, a tensor crossing a 2048-element span boundary,
    a whole empty span between two tensors, a zero-size tensor in the middle."""
    rng = np.random.RandomState(0)
    sizes, offsets = [], []
    pos = 24
    for i in range(106):
        n = 2 * int(rng.randint(0, 400)) + 1
        if i == 50:
            n = 0
        if i == 3:
            n = 3001  # longer than a span: crosses at least one boundary
        if i == 80:
            n = 101
        if i == 60:
            # a gap that holds one whole 2048-element span without any tensor
            pos = (pos + 2047) // 2048 * 2048 + 2048 + 24
        if i == 80:
            # starts 5 elements before a span boundary
            pos = (pos + 2047) // 2048 * 2048 + 2048 - 5
        offsets.append(pos)
        sizes.append(n)
        pos += n + int(rng.randint(0, 40))
    return sizes, offsets, pos + 3000


@pytest.mark.parametrize("dt", [BF16, torch.float32], ids=["bf16", "f32"])
def test_flatten_scale_sentinels(cuda, dt):
    m = _m()
    g = _gen(cuda)
    sizes, offsets, total = _bucket_layout()
    assert offsets[0] == 24 and sizes[50] == 0 and len(sizes) == 106
    assert (offsets[60] - 24) % 2048 == 0 and offsets[60] - 24 - 2048 >= offsets[59] + sizes[59]
    assert offsets[80] % 2048 == 2043 and sizes[80] > 5
    ts = [torch.randn(n, device=cuda, generator=g).to(dt) for n in sizes]  # fresh allocations
    flat = torch.full((total,), SENT, device=cuda, dtype=dt)
    scale = f32(0.3)
    m.flatten_scale(ts, flat, offsets, scale, False)
    want = torch.full((total,), SENT, device=cuda, dtype=dt)
    s = torch.tensor(scale, device=cuda, dtype=torch.float32)
    for t, o in zip(ts, offsets):
        want[o:o + t.numel()] = (t.float() * s).to(dt)
    assert same_bits(flat[:24], want[:24]), "elements below the first offset were written"
    assert same_bits(flat, want)


@pytest.mark.parametrize("dt", [BF16, torch.float32], ids=["bf16", "f32"])
def test_unflatten_sentinels(cuda, dt):
    m = _m()
    g = _gen(cuda, 1)
    sizes, offsets, total = _bucket_layout()
    flat = torch.randn(total, device=cuda, generator=g).to(dt)
    slot = 4096  # every tensor starts at a multiple of 1024 elements, sentinels on both sides
    big = torch.full((1024 + slot * len(sizes),), SENT, device=cuda, dtype=dt)
    ts = [big[1024 + i * slot:1024 + i * slot + n] for i, n in enumerate(sizes)]
    flat0 = flat.clone()
    m.flatten_scale(ts, flat, offsets, 1.0, True)
    want = torch.full_like(big, SENT)
    for i, (n, o) in enumerate(zip(sizes, offsets)):
        want[1024 + i * slot:1024 + i * slot + n] = flat0[o:o + n]
    assert same_bits(big, want)
    assert same_bits(flat, flat0)


# ---------------------------------------------------------------------------------------------
# 1. AdamW / SGD against float64
# ---------------------------------------------------------------------------------------------
ADAMW_N = 2 * 4_194_304 + 3 * 1024  # two full grid trips + a tail (one + a tail for variant 3)
CLIP_MODES = {"active": (4.0, 1.0), "inactive": (0.25, 1.0), "disabled": (math.nan, -1.0)}


class _AdamWCase:
    """Inputs, and the float64 reference and the kernels' results for one clip mode at a time (asking
    for another mode drops the last one's)."""

    def __init__(self, dev):
        self.dev = dev
        g = _gen(dev, 7)
        n = ADAMW_N
        gr = torch.randn(n, device=dev, generator=g)
        gr[torch.rand(n, device=dev, generator=g) < 0.01] = 0.0
        gr[:3] = 0.0
        self.g = gr.bfloat16()
        self.m0 = 0.1 * torch.randn(n, device=dev, generator=g)
        self.v0 = (0.1 * torch.randn(n, device=dev, generator=g)) ** 2
        self.w0 = 0.02 * torch.randn(n, device=dev, generator=g)
        dec = torch.randint(0, 2, (n // 1024,), device=dev, generator=g).float()
        dec[0], dec[1] = 1.0, 0.0  # elements 1023 and 1024 differ
        self.dec = dec
        t = 7
        self.hp = dict(lr=f32(3e-4), b1=f32(0.9), b2=f32(0.95), eps=f32(1e-8), wd=f32(0.1))
        self.hp["bc1"] = f32(1.0 - 0.9 ** t)
        self.hp["bc2"] = f32(1.0 - 0.95 ** t)
        self.grad_scale = 0.25
        self.drop()

    def drop(self):
        self._mode, self._ref, self._run = None, None, {}

    def _enter(self, mode):
        if mode != self._mode:
            self.drop()
            self._mode = mode

    def ref(self, mode):
        self._enter(mode)
        if self._ref is None:
            normsq, clip = CLIP_MODES[mode]
            c = clip_coef(normsq, clip, self.grad_scale)
            dec = self.dec.double().repeat_interleave(1024)
            w, m, v, upd = adamw_ref(self.w0.double(), self.m0.double(), self.v0.double(), self.g.double(), dec, c,
                                     **self.hp)
            hp = self.hp
            bm = 4 * U * (hp["b1"] * self.m0.double().abs() + (1.0 - hp["b1"]) * (c * self.g.double()).abs())
            bv = 8 * U * v
            # the fixed count of roundings on w0·shrink and on upd, relative to upd ...
            bw_rel = 4 * U * self.w0.double().abs() + 32 * U * hp["lr"] * upd.abs()
            # ... and the error bm that the moment bound allows m, carried through m̂ / (√v̂ + eps): it is
            # relative to |b1·m0| + |(1−b1)·c·g|, not to |m|, so where the two terms cancel no count of
            # roundings relative to upd covers it
            bw = bw_rel + hp["lr"] * (bm / hp["bc1"]) / (v.sqrt() / math.sqrt(hp["bc2"]) + hp["eps"])
            self._ref = dict(w=w, m=m, v=v, bm=bm, bv=bv, bw=bw, bw_rel=bw_rel)
        return self._ref

    def run(self, variant, mode):
        self._enter(mode)
        if variant not in self._run:
            m = _m()
            normsq, clip = CLIP_MODES[mode]
            ns = torch.full((2,), normsq, device=self.dev, dtype=torch.float32)
            p = torch.zeros(ADAMW_N, device=self.dev, dtype=BF16)
            w, m1, m2 = self.w0.clone(), self.m0.clone(), self.v0.clone()
            hp = self.hp
            m.set_adamw_variant(variant)
            try:
                m.adamw_flat(p, self.g, w, m1, m2, self.dec, ns, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"],
                             hp["bc1"], hp["bc2"], self.grad_scale, clip)
                torch.cuda.synchronize()
            finally:
                m.set_adamw_variant(int(os.environ.get("PDO_ADAMW") or 2))
            self._run[variant] = dict(p=p, w=w, m=m1, v=m2)
        return self._run[variant]


@pytest.fixture(scope="module")
def adamw_case(cuda):
    case = _AdamWCase(cuda)
    yield case
    case.drop()


# the clip mode is the outer parameter: all of a mode's tests run before the next mode's
@pytest.mark.parametrize("variant", [1, 2, 3, "agree"])
@pytest.mark.parametrize("mode", list(CLIP_MODES))
def test_adamw_flat_fp64(adamw_case, mode, variant):
    """One step at t = 7 against the float64 textbook step on the same fp32 inputs:
    |m − m_ref| ≤ B_m = 4u·(b1|m0| + (1−b1)|c·g|),  |v − v_ref| ≤ 8u·v_ref,
    |w − w_ref| ≤ 4u·|w0| + 32u·lr·|upd_ref| + lr·(B_m / bc1) / (√(v_ref / bc2) + eps),
    and the bf16 copy is the rounding of the kernel's own fp32 master.  "agree": the three variants'
    m and v differ from each other by no more than the same bounds.

    The last term of the w bound is B_m carried through upd = m̂ / (√v̂ + eps).  Without it the bound
    takes m's error for a few u of |m|; fp32 roundings of b1·m0 and (1−b1)·c·g leave a few u of
    |b1·m0| + |(1−b1)·c·g|, which is many times |m| where the terms cancel.  The test prints the worst
    error against the bound without that term as well: no fp32 kernel, the IEEE one included, stays
    under it."""
    ref = adamw_case.ref(mode)
    if variant == "agree":
        runs = {k: adamw_case.run(k, mode) for k in (1, 2, 3)}
        for a, b in ((1, 2), (1, 3), (2, 3)):
            rm = _worst((runs[a]["m"].double() - runs[b]["m"].double()).abs(), ref["bm"])
            rv = _worst((runs[a]["v"].double() - runs[b]["v"].double()).abs(), ref["bv"])
            print(f"adamw variants {a} vs {b} clip {mode}: worst diff / bound  m {rm:.3f}  v {rv:.3f}")
            assert rm <= 1.0 and rv <= 1.0
        return
    got = adamw_case.run(variant, mode)
    rm = _worst((got["m"].double() - ref["m"]).abs(), ref["bm"])
    rv = _worst((got["v"].double() - ref["v"]).abs(), ref["bv"])
    werr = (got["w"].double() - ref["w"]).abs()
    rw, rw_rel = _worst(werr, ref["bw"]), _worst(werr, ref["bw_rel"])
    print(f"adamw variant {variant} clip {mode}: worst err / bound  m {rm:.3f}  v {rv:.3f}  w {rw:.3f}"
          f"  (w without the carried moment term {rw_rel:.3f})")
    assert torch.equal(got["p"], got["w"].bfloat16())
    assert rm <= 1.0
    assert rv <= 1.0
    assert rw <= 1.0


def test_sgd_flat_fp64(cuda):
    """n past the 2048-block grid's first trip; |buf − ref| ≤ 4u·(|mom·buf0| + |g·sc| + |wd·w0|) = B,
    |w − ref| ≤ 2u·|w0| + lr·B + 2u·lr·|buf_ref|."""
    m = _m()
    g = _gen(cuda, 3)
    n = 2_097_152 + 3 * 1024
    w0 = 0.05 * torch.randn(n, device=cuda, generator=g)
    gr = torch.randn(n, device=cuda, generator=g)
    buf0 = 0.1 * torch.randn(n, device=cuda, generator=g)
    dec = (torch.arange(n // 1024, device=cuda) % 2 == 0).float()  # elements 1023 and 1024 differ
    lr, mom, wd, sc = f32(0.1), f32(0.9), f32(1e-4), 0.25
    w, buf = w0.clone(), buf0.clone()
    m.sgd_flat(w, gr, buf, dec, lr, mom, wd, sc)
    w_ref, buf_ref = sgd_ref(w0.double(), buf0.double(), gr.double(), dec.double().repeat_interleave(1024), lr, mom,
                             wd, sc)
    B = 4 * U * ((mom * buf0.double()).abs() + (gr.double() * sc).abs() + (wd * w0.double()).abs())
    Bw = 2 * U * w0.double().abs() + lr * B + 2 * U * lr * buf_ref.abs()
    rb = _worst((buf.double() - buf_ref).abs(), B)
    rw = _worst((w.double() - w_ref).abs(), Bw)
    print(f"sgd: worst err / bound  buf {rb:.3f}  w {rw:.3f}")
    assert rb <= 1.0 and rw <= 1.0


# ---------------------------------------------------------------------------------------------
# 2. gradient-norm kernels, exact
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def norm_grad(cuda):
    return _ints((300_008,), -2, 2, cuda, _gen(cuda, 11))


def _chunk_sums(g, chunk):
    n = g.numel()
    K = (n + chunk - 1) // chunk
    sq = torch.zeros(K * chunk, device=g.device, dtype=torch.float64)
    sq[:n] = g.double() ** 2
    return sq.view(K, chunk).sum(1)


@pytest.mark.parametrize("chunk", [8, 2056, 65536])
def test_sumsq_chunks_exact(cuda, norm_grad, chunk):
    m = _m()
    want = _chunk_sums(norm_grad, chunk)
    K = want.numel()
    part = torch.full((K,), -7.0, device=cuda)
    m.sumsq_chunks(norm_grad, part, chunk, 0, K)
    assert torch.equal(part.double(), want)  # the short last chunk included
    k0, k1 = max(1, K // 3), K - 1
    assert 0 < k0 < k1 < K
    sub = torch.full((K,), -7.0, device=cuda)
    m.sumsq_chunks(norm_grad, sub, chunk, k0, k1)
    assert torch.equal(sub[k0:k1].double(), want[k0:k1])
    assert bool((sub[:k0] == -7.0).all()) and bool((sub[k1:] == -7.0).all())
    out = torch.full((2,), -7.0, device=cuda)
    m.sumsq_total(part, out, 0.5)
    assert float(out[0]) == 0.25 * float(want.sum()) and float(out[1]) == -7.0


def test_sumsq_total_second_stride(cuda):
    m = _m()
    part = _ints((1500,), 0, 100, cuda, _gen(cuda, 12), torch.float32)
    part[1024:] += 1000.0  # the second stride of the 1024-thread kernel carries weight
    out = torch.zeros(2, device=cuda)
    m.sumsq_total(part, out, 0.5)
    assert float(out[0]) == 0.25 * float(part.double().sum())


@pytest.mark.parametrize("n", [8, 4_194_312])
def test_sumsq_exact(cuda, n):
    m = _m()
    g = _ints((n,), -1, 1, cuda, _gen(cuda, 13))
    g[-1] = 1.0  # the lone vector of the second grid trip counts
    out = torch.full((2,), -7.0, device=cuda)
    m.sumsq(g, out, 0.5)
    assert float(out[0]) == 0.25 * float((g.double() ** 2).sum()) and float(out[1]) == -7.0


def test_sumsq_rejections(cuda):
    m = _m()
    g12 = torch.zeros(12, device=cuda, dtype=BF16)
    g16 = torch.zeros(16, device=cuda, dtype=BF16)
    out = torch.zeros(2, device=cuda)
    part = torch.zeros(4, device=cuda)
    with pytest.raises(RuntimeError):
        m.sumsq(g12, out, 1.0)
    with pytest.raises(RuntimeError):
        m.sumsq_chunks(g12, part, 8, 0, 1)
    with pytest.raises(RuntimeError):
        m.sumsq_chunks(g16, part, 12, 0, 1)


# ---------------------------------------------------------------------------------------------
# 3. column sums, exact
# ---------------------------------------------------------------------------------------------
BIAS_SHAPES = [(N, F) for N in (1, 7, 257, 513) for F in (8, 520, 3072)]


@pytest.mark.parametrize("N,F", BIAS_SHAPES)
def test_bias_grad_exact(cuda, N, F):
    m = _m()
    g = _gen(cuda, N * 10007 + F)
    dy = _ints((N, F), -2, 2, cuda, g)
    s = dy.double().sum(0)
    assert same_bits(m.bias_grad(dy), s.bfloat16())
    out0 = _ints((F,), -8, 8, cuda, g)
    out = out0.clone()
    ret = m.bias_grad(dy, out)
    assert ret.data_ptr() == out.data_ptr()
    assert same_bits(out, (out0.double() + s).bfloat16())


@pytest.mark.parametrize("N,F", BIAS_SHAPES)
def test_bias_grad_needles(cuda, N, F):
    m = _m()
    dy = torch.zeros(N, F, device=cuda, dtype=BF16)
    dy[0, 0] = 1.0
    dy[N - 1, F - 1] = 1.0
    assert same_bits(m.bias_grad(dy), dy.double().sum(0).bfloat16())


LN_SHAPES = [(16, 1600), (64, 768), (1024, 64), (1040, 768), (4096, 1024)]  # G = 1, 4, 64, 65, 256


class _LnJob:
    def __init__(self, dev, g, N, C, rbias=False):
        self.N, self.C, self.rbias = N, C, rbias
        self.dy = _ints((N, C), -2, 2, dev, g)
        self.x = _ints((N, C), -2, 2, dev, g)
        # dx is not under test; with w = 0 the fused residual-bias gradient is Σ dres exactly
        self.w = torch.zeros(C, device=dev, dtype=BF16) if rbias else _ints((C,), -2, 2, dev, g)
        self.mean = torch.zeros(N, device=dev)
        self.rstd = torch.ones(N, device=dev)
        self.sums = [(self.dy.double() * self.x.double()).sum(0), self.dy.double().sum(0)]
        if rbias:
            self.dres = _ints((N, C), -2, 2, dev, g)
            self.sums.append(self.dres.double().sum(0))

    def launch(self, m, dests):
        if self.rbias:
            m.layernorm_bwd_add(self.dy, self.x, self.w, self.mean, self.rstd, self.dres, True, dests)
        else:
            m.layernorm_bwd(self.dy, self.x, self.w, self.mean, self.rstd, dests)


def test_colsum_deferred_equals_immediate(cuda):
    """33 norm-weight gradient jobs (> COLSUM_BATCH), level-1-only and level-2 jobs alternating, two jobs on
    one destination and one three-segment job: deferred = immediate = float64, bit for bit."""
    m = _m()
    g = _gen(cuda, 21)
    jobs = [_LnJob(cuda, g, *LN_SHAPES[i % 5]) for i in range(30)]
    jobs += [_LnJob(cuda, g, 64, 768), _LnJob(cuda, g, 1040, 768)]  # these two share one destination
    jobs.append(_LnJob(cuda, g, 1040, 768, rbias=True))
    base = [[_ints((j.C,), -8, 8, cuda, g) for _ in j.sums] for j in jobs]
    base[31] = base[30]

    def run(defer):
        dests = [[b.clone() for b in bs] for bs in base]
        dests[31] = dests[30]
        prev = m.colsum_defer(defer)
        try:
            for j, d in zip(jobs, dests):
                j.launch(m, d)
            if defer:
                assert m.colsum_pending() == len(jobs)
                m.colsum_flush()
            assert m.colsum_pending() == 0
        finally:
            m.colsum_defer(prev)
        torch.cuda.synchronize()
        return dests

    now, later = run(False), run(True)
    for i, j in enumerate(jobs):
        if i == 31:
            continue
        for k, s in enumerate(j.sums):
            want = (base[i][k].double() + s).bfloat16()
            if i == 30:  # two contributions added in order, each rounded
                want = (want.double() + jobs[31].sums[k]).bfloat16()
            assert same_bits(now[i][k], want), f"immediate: job {i} (N {j.N}, C {j.C}) segment {k}"
            assert same_bits(later[i][k], want), f"deferred: job {i} (N {j.N}, C {j.C}) segment {k}"
            assert same_bits(later[i][k], now[i][k])


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("n", [8, 3 * 2048 + 8])
@pytest.mark.parametrize("s", [1, 8, 9, 16])
def test_splitk_add_exact(cuda, s, n, acc):
    m = _m()
    g = _gen(cuda, s * 31 + n)
    part = _ints((s, n), -100, 100, cuda, g)
    out0 = _ints((n,), -8, 8, cuda, g)
    out = out0.clone()
    m.splitk_add(part, out, acc)
    want = part.double().sum(0) + (out0.double() if acc else 0.0)
    assert same_bits(out, want.bfloat16())


def test_splitk_add_rejections(cuda):
    m = _m()
    with pytest.raises(RuntimeError):
        m.splitk_add(torch.zeros(17, 8, device=cuda, dtype=BF16), torch.zeros(8, device=cuda, dtype=BF16), False)
    with pytest.raises(RuntimeError):
        m.splitk_add(torch.zeros(2, 12, device=cuda, dtype=BF16), torch.zeros(12, device=cuda, dtype=BF16), False)


# ---------------------------------------------------------------------------------------------
# 4. elementwise bucket kernels
# ---------------------------------------------------------------------------------------------
EW_SIZES = [8, 4_194_312]  # one vector; a second grid trip of one vector


def _scaled(x, s):
    """bf16(fp32(x · fp32(s))): the product of an 8-bit and a 24-bit significand is exact in float64."""
    return (x.double() * f32(s)).float().bfloat16()


@pytest.mark.parametrize("n", EW_SIZES)
@pytest.mark.parametrize("s", [0.5, 1.0 / 3.0])
def test_scale_exact(cuda, n, s):
    m = _m()
    x0 = torch.randn(n, device=cuda, generator=_gen(cuda, 31)).bfloat16()
    x = x0.clone()
    m.scale_(x, s)
    assert same_bits(x, _scaled(x0, s))
    x = x0.clone()
    m.scale_dev_(x, torch.tensor([s], device=cuda, dtype=torch.float32))
    assert same_bits(x, _scaled(x0, s))


@pytest.mark.parametrize("n", EW_SIZES)
def test_scale_dev_one_leaves_bits(cuda, n):
    m = _m()
    x0 = torch.randn(n, device=cuda, generator=_gen(cuda, 32)).bfloat16()
    x0[1] = -0.0
    b = x0.view(torch.int16)
    b[2], b[3], b[n - 1] = 0x7FC1, -1, 0x7F81  # NaN bit patterns, quiet and signalling
    x = x0.clone()
    m.scale_dev_(x, torch.ones(1, device=cuda))
    assert torch.equal(x.view(torch.int16), x0.view(torch.int16))


@pytest.mark.parametrize("n", EW_SIZES)
def test_axpy_dev_exact(cuda, n):
    m = _m()
    g = _gen(cuda, 33)

    def val():
        mag = (0.5 + 1.5 * torch.rand(n, device=cuda, generator=g)).bfloat16().clamp(max=1.9921875)
        return torch.where(torch.rand(n, device=cuda, generator=g) < 0.5, -mag, mag)

    x, y0 = val(), val()
    s = torch.tensor([0.3], device=cuda, dtype=torch.float32)
    y = y0.clone()
    m.axpy_dev_(y, x, s)
    # y + s·x is exact in float64 (24-bit × 8-bit product, an 8-bit addend a few binades away), so
    # rounding it to fp32 is the fused multiply-add's one rounding
    want = (y0.double() + s.double() * x.double()).float().bfloat16()
    assert same_bits(y, want)


@pytest.mark.parametrize("n", EW_SIZES)
def test_fold_zero_exact(cuda, n):
    m = _m()
    g = _gen(cuda, 34)
    g0 = torch.randn(n, device=cuda, generator=g).bfloat16()
    h0 = torch.randn(n, device=cuda, generator=g).bfloat16()
    h0[::5] = -g0[::5]
    gg, h = g0.clone(), h0.clone()
    m.fold_zero(gg, h)
    assert same_bits(gg, (g0.double() + h0.double()).float().bfloat16())
    assert int(h.view(torch.int16).abs().max()) == 0  # all +0.0


@pytest.mark.parametrize("n", EW_SIZES)
@pytest.mark.parametrize("s", [0.5, 1.0 / 3.0])
def test_cast_scale_bf16_f32_exact(cuda, n, s):
    m = _m()
    src = torch.randn(n, device=cuda, generator=_gen(cuda, 35)).bfloat16()
    dst = torch.full((n,), SENT, device=cuda)
    m.cast_scale_bf16_f32(src, dst, s)
    assert same_bits(dst, (src.double() * f32(s)).float())


def _halfway_f32(dev, n, gen):
    """fp32 values on, one ulp below and one ulp above the midpoint of two bf16 neighbours: random sign,
    normal exponent and bf16 significand (so even and odd lower neighbours), low half 0x7FFF/0x8000/0x8001."""
    sign = torch.randint(0, 2, (n,), device=dev, generator=gen, dtype=torch.int64)
    expo = torch.randint(1, 0xFE, (n,), device=dev, generator=gen, dtype=torch.int64)
    mant = torch.randint(0, 128, (n,), device=dev, generator=gen, dtype=torch.int64)
    low = torch.randint(0, 3, (n,), device=dev, generator=gen, dtype=torch.int64) + 0x7FFF
    bits = (sign << 31) | (expo << 23) | (mant << 16) | low
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)
    return bits.to(torch.int32).view(torch.float32)


@pytest.mark.parametrize("n", EW_SIZES)
def test_cast_f32_bf16_ties(cuda, n):
    m = _m()
    src = _halfway_f32(cuda, n, _gen(cuda, 36))
    # 1 + 2^-8 (even lower neighbour: down), 1 + 3·2^-8 (odd: up), both signs, and one ulp to either side
    hand = torch.tensor([0x3F808000, 0x3F818000, -0x407F8000, -0x407E8000, 0x3F807FFF, 0x3F808001, 0x3F817FFF,
                         0x3F818001], dtype=torch.int32, device=cuda).view(torch.float32)
    src[:8] = hand
    dst = torch.zeros(n, device=cuda, dtype=BF16)
    m.cast_f32_bf16(src, dst)
    assert [float(v) for v in dst[:4]] == [1.0, 1.015625, -1.0, -1.015625]
    assert same_bits(dst, src.bfloat16())


def _transpose_table():
    shapes = [(64, 64), (64, 192), (320, 128), (128, 64)]
    rows, tile, so, do = [], 0, 1024, 2048
    for R, C in shapes:
        rows.append([tile, so, do, R, C])
        tile += (R // 64) * (C // 64)
        so = (so + R * C + 1023) // 1024 * 1024 + 1024  # a gap after every matrix
        do = (do + R * C + 1023) // 1024 * 1024 + 3072
    return rows, tile, so, do


def test_transpose_batched_exact(cuda):
    m = _m()
    rows, tiles, nsrc, ndst = _transpose_table()
    src = torch.randn(nsrc, device=cuda, generator=_gen(cuda, 37)).bfloat16()
    dst = torch.full((ndst,), SENT, device=cuda, dtype=BF16)
    host = torch.tensor(rows, dtype=torch.int64)
    m.transpose_batched(src, dst, host.to(cuda), host, tiles)
    want = torch.full_like(dst, SENT)
    for _, so, do, R, C in rows:
        want[do:do + R * C] = src[so:so + R * C].view(R, C).t().reshape(-1)
    assert same_bits(dst, want)


def test_transpose_batched_rejections(cuda):
    m = _m()
    rows, tiles, nsrc, ndst = _transpose_table()
    src = torch.zeros(nsrc, device=cuda, dtype=BF16)
    dst = torch.full((ndst,), SENT, device=cuda, dtype=BF16)
    host = torch.tensor(rows, dtype=torch.int64)
    dev = host.to(cuda)
    with pytest.raises(RuntimeError):
        m.transpose_batched(src, dst, dev, host[:-1].contiguous(), tiles)  # host does not mirror the device table
    with pytest.raises(RuntimeError):
        m.transpose_batched(src, dst, dev, host, tiles + 1)
    bad = host.clone()
    bad[3, 2] = ndst - 64  # the last matrix would run past dst
    with pytest.raises(RuntimeError):
        m.transpose_batched(src, dst, bad.to(cuda), bad, tiles)
    bad = host.clone()
    bad[1, 1] = -1024
    with pytest.raises(RuntimeError):
        m.transpose_batched(src, dst, bad.to(cuda), bad, tiles)
    torch.cuda.synchronize()
    assert bool((dst == SENT).all())  # nothing was launched


# ---------------------------------------------------------------------------------------------
# 5. cross-entropy edges against float64
# ---------------------------------------------------------------------------------------------
# (8, 5): a row of one vector; (6152, 6150): 769 vectors, one lane takes one trip of the 4-deep loop;
# (53248, 53248): the register kernel at its widest, no padding; (53256, 53250): the two-read kernel
XENT_SHAPES = [(8, 5), (6152, 6150), (53248, 53248), (53256, 53250)]


def _xent_inputs(dev, Vp, V, all_ignored=False):
    g = _gen(dev, Vp)
    pad = V + (Vp - V) // 2 if Vp > V else -100  # a target in the padding: ignored
    if all_ignored:
        tgt = torch.tensor([-100, pad, -100], device=dev)
    else:
        tgt = torch.tensor([0, V - 1, V // 2, -100, pad, min(3, V - 1)], device=dev)
    N = tgt.numel()
    lg = (2.0 * torch.randn(N, Vp, device=dev, generator=g)).bfloat16()
    lg[1] = -80.0  # a spike on the target over a flat background
    lg[1, V - 1] = 80.0
    lg[:, V:] = 100.0
    return lg, tgt


def _check_dlogits(got, ref, scale, tgt, V, what):
    err = (got.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * scale
    r = float((err / bound).max()) if scale > 0 else (0.0 if float(err.max()) == 0.0 else math.inf)
    print(f"{what}: worst dlogits err / bound {r:.3f}")
    assert not bool(got.isnan().any())
    assert r <= 1.0, what
    dead = ~((tgt >= 0) & (tgt < V))
    assert bool((got[dead] == 0).all()), what + ": a row without a valid target has a gradient"
    assert bool((got[:, V:] == 0).all()), what + ": a padding column has a gradient"


@pytest.mark.parametrize("Vp,V", XENT_SHAPES)
def test_xent_edges_fp64(cuda, Vp, V):
    m = _m()
    lg, tgt = _xent_inputs(cuda, Vp, V)
    dl = 0.5
    loss_ref, lse_ref, d_ref, cnt = xent_ref(lg, tgt, V, dl)
    assert cnt == 4
    dloss = torch.tensor([dl], device=cuda)
    for inplace in (False, True):
        x = lg.clone()
        loss, lse, stats = m.xent_fwd(x, tgt, V)
        assert float(stats[1]) == cnt
        assert abs(float(loss) - loss_ref) <= 1e-3 * max(1.0, loss_ref)
        lerr = (lse.double() - lse_ref).abs() / lse_ref.abs().clamp_min(1.0)
        print(f"xent_fwd ({Vp}, {V}): loss {float(loss):.6f} ref {loss_ref:.6f}, worst lse err {float(lerr.max()):.2e}")
        assert bool((lerr <= 1e-4).all())
        d = m.xent_bwd(x, tgt, lse, dloss, stats, V, inplace)
        if inplace:
            assert d.data_ptr() == x.data_ptr()
        else:
            assert same_bits(x, lg)
        _check_dlogits(d, d_ref, dl / cnt, tgt, V, f"xent_bwd ({Vp}, {V}) inplace={inplace}")
    x = lg.clone()
    _, _, d1_ref, _ = xent_ref(lg, tgt, V, 1.0)
    loss = m.xent_fused(x, tgt, torch.tensor([1.0 / cnt], device=cuda), V)
    assert abs(float(loss) - loss_ref) <= 1e-3 * max(1.0, loss_ref)
    _check_dlogits(x, d1_ref, 1.0 / cnt, tgt, V, f"xent_fused ({Vp}, {V})")


@pytest.mark.parametrize("Vp,V", XENT_SHAPES)
def test_xent_all_targets_ignored(cuda, Vp, V):
    m = _m()
    lg, tgt = _xent_inputs(cuda, Vp, V, all_ignored=True)
    zero = torch.zeros_like(lg, dtype=torch.float64)
    for inplace in (False, True):
        x = lg.clone()
        loss, lse, stats = m.xent_fwd(x, tgt, V)
        assert float(loss) == 0.0 and float(stats[1]) == 0.0
        d = m.xent_bwd(x, tgt, lse, torch.ones(1, device=cuda), stats, V, inplace)
        _check_dlogits(d, zero, 0.0, tgt, V, f"xent_bwd ({Vp}, {V}) all ignored")
    x = lg.clone()
    loss = m.xent_fused(x, tgt, torch.ones(1, device=cuda), V)
    assert float(loss) == 0.0
    _check_dlogits(x, zero, 0.0, tgt, V, f"xent_fused ({Vp}, {V}) all ignored")
