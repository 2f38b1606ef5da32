"""LARS over the flat arena (csrc/hip/lars.hip, FlatLARS): kernels against float64, bits, the tiny trainer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (elements, decayed, zeroed): a partial chunk, one chunk, a second chunk of one element, 9.5 chunks,
# 301 chunks (more than pass B's 256 threads: every level of its fold), two zero norms (λ = 1)
SLOTS = [(64, False, ""), (1024, True, ""), (1025, True, ""), (9 * 1024 + 512, False, ""),
         (300 * 1024 + 7, True, ""), (2053, True, "g"), (700, True, "w"), (64, True, "")]
LR, MOM, WD, COEFF, EPS, SC = (float(np.float32(x)) for x in (0.1, 0.9, 1e-4, 0.001, 0.0, 0.3))


def _run(a, lr=LR, lr_dev=None):
    from paddle_operator_amd import _native
    w, v = a["w"].clone(), a["v"].clone()
    ratio = torch.full((w.numel() // 1024,), -1.0, device=w.device)
    _native.require_hip().lars_flat(w, a["g"], v, a["decay"], ratio, torch.zeros(2 * ratio.numel(), device=w.device),
                                    a["host"].to(w.device), a["host"], lr, MOM, WD, COEFF, EPS, SC, lr_dev)
    return w, v, ratio


@pytest.fixture(scope="module")
def case(cuda):
    """w, g, v: random inside the slots, zero in the padding; one run of the kernels from them."""
    gen = torch.Generator(device=cuda).manual_seed(5)
    rows, chunks = [], 0
    for n, dec, _ in SLOTS:
        rows.append((chunks, -(-n // 1024), int(dec)))
        chunks += rows[-1][1]
    w, g, v = (torch.zeros(chunks * 1024, device=cuda) for _ in range(3))
    decay = torch.zeros(chunks, device=cuda)
    for (n, dec, zero), (c0, K, _) in zip(SLOTS, rows):
        for t, scale in ((w, 0.05), (g, 1.0), (v, 0.01)):
            t[c0 * 1024:c0 * 1024 + n] = scale * torch.randn(n, device=cuda, generator=gen)
        if zero:
            (g if zero == "g" else w)[c0 * 1024:c0 * 1024 + n] = 0
        decay[c0:c0 + K] = float(dec)
    a = dict(w=w, g=g, v=v, decay=decay, host=torch.tensor(rows, dtype=torch.int32))
    a["out"] = _run(a)
    return a


@pytest.mark.parametrize("i", range(len(SLOTS)), ids=[f"{n}{'d' if d else ''}{z}" for n, d, z in SLOTS])
def test_lars_flat_fp64(case, i):
    """λ: lars.hip's header counts 31 + ceil(K / 256) additions on the longest path of a K-chunk
    tensor's sums (pass A: 16 per lane + 6 across lanes; pass B: ceil(K / 256) per lane + 6 across
    lanes + 3 across waves), so |λ − λ64| ≤ (31 + ceil(K / 256) + 4)·u·λ64.  v, w against float64 with
    the kernel's λ: test_sgd_flat_fp64's bounds with one more rounding (lr·λ) and the rate inside v:
    |v − ref| ≤ 5u·(|mom·v0| + r·|g·sc| + r·|wd·w0|) = B, |w − ref| ≤ 2u·|w0| + B + 2u·|v_ref|."""
    (n, dec, _), (c0, K, _) = SLOTS[i], case["host"][i].tolist()
    o = c0 * 1024
    w0, g, v0 = (case[k][o:o + n].double() for k in ("w", "g", "v"))
    w, v, ratio = case["out"]
    lam = float(ratio[c0])
    assert bool((ratio[c0:c0 + K] == lam).all())
    W, G = float(w0.norm()), float((g * SC).norm())
    want = COEFF * W / (G + WD * W + EPS) if dec and W > 0 and G > 0 else 1.0
    bound = (31 + -(-K // 256) + 4) * U * want
    r = LR * lam
    v_ref = MOM * v0 + r * (g * SC + WD * float(dec) * w0)
    B = 5 * U * ((MOM * v0).abs() + r * (g * SC).abs() + r * (WD * w0).abs())
    Bw = 2 * U * w0.abs() + B + 2 * U * v_ref.abs()
    ev, ew = (v[o:o + n].double() - v_ref).abs(), (w[o:o + n].double() - (w0 - v_ref)).abs()
    print(f"slot {n}: λ {lam:.9g} want {want:.9g} err/bound {abs(lam - want) / bound:.3f}; worst err / bound"
          f"  v {float((ev / B.clamp_min(1e-300)).max()):.3f}  w {float((ew / Bw.clamp_min(1e-300)).max()):.3f}")
    assert (lam == 1.0) if want == 1.0 else abs(lam - want) <= bound
    assert bool((ev <= B).all()) and bool((ew <= Bw).all())
    for t in (w, v):  # the padding: bitwise zero
        assert not bool(t[o + n:o + K * 1024].view(torch.int32).any())


@pytest.mark.parametrize("mode", ["value", "dev"])
def test_lars_flat_bitwise(case, mode):
    """Same bits from two runs and from both rate routes; a by-value rate beside lr_dev is ignored."""
    kw = dict(lr=123.0, lr_dev=torch.tensor([LR], device=case["w"].device)) if mode == "dev" else {}
    for x, y, z in zip(_run(case, **kw), _run(case, **kw), case["out"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert torch.equal(x.view(torch.int32), z.view(torch.int32))


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = tmp_path_factory.mktemp("lars-data")
    np.save(d / "images.npy", np.random.default_rng(1).integers(0, 256, (32, 40, 40, 3), dtype=np.uint8))
    np.save(d / "labels.npy", (np.arange(32) % 10).astype(np.int16))
    return str(d)


@pytest.fixture
def deterministic_convs():
    """The tiny model's channels are no multiples of 64: its convolutions run in the framework, whose
    default weight-gradient algorithms vary in the last bit from run to run (under SGD just as often)."""
    old, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    yield
    torch.backends.cudnn.deterministic = old


def _trained(cuda, images, steps, optimizer="lars", graph=False, resume=None):
    from paddle_operator_amd.workloads.resnet import ResNetTrainer
    torch.manual_seed(0)
    t = ResNetTrainer(8, cuda, tiny=True, graph=graph, optimizer=optimizer, data=images, data_seed=3, lr=0.5,
                      lr_schedule="cosine", lr_warmup=2, lr_decay_steps=5)
    if resume is not None:
        t.load_state_dict(resume)
    t.losses = [float(t.step()) for _ in range(steps)]
    torch.cuda.synchronize()
    t.close()
    return t


def test_lars_trainer_graph_and_resume(cuda, images, deterministic_convs):
    """5 steps under a cosine schedule: eager, captured (2 eager, the capture, 2 replays) and resumed
    from a checkpoint after step 2 give the same bits; the other optimizer's checkpoint is refused."""
    e, g, half = _trained(cuda, images, 5), _trained(cuda, images, 5, graph=True), _trained(cuda, images, 2)
    sd = half.state_dict()  # half takes no further step: its tensors are the checkpoint
    r = _trained(cuda, images, 3, resume=sd)
    assert e._graph is None and g._graph is not None, "graph mode not taken"
    assert e.losses == g.losses == half.losses + r.losses and all(np.isfinite(e.losses)), (e.losses, g.losses)
    for t in (g, r):
        assert torch.equal(e.flat.params, t.flat.params) and torch.equal(e.opt.buf, t.opt.buf)
        assert torch.equal(e.opt.ratio, t.opt.ratio) and t.opt.step_count == 5
    assert float(e.opt.ratio.min()) > 0 and bool((e.opt.ratio != 1).any())
    sgd = _trained(cuda, images, 0, optimizer="sgd")
    assert sd["optimizer"] == "lars" and "optimizer" not in sgd.state_dict()
    for t, other in ((sgd, sd), (r, sgd.state_dict())):
        with pytest.raises(ValueError, match="checkpoint written with"):
            t.load_state_dict(other)
