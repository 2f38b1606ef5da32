"""quant_e4m3_grouped against ops.ref_quant_e4m3 bit for bit, its rejections, the trainer with the arena copies on / off."""
import pytest
import torch

from paddle_operator_amd import _native, ops
from paddle_operator_amd.models.gpt2 import GPT2Config
from paddle_operator_amd.ops import fp8 as fp8_ops
from paddle_operator_amd.parallel.flat import WQ_CHUNK, wq_table
from paddle_operator_amd.train import GPT2Trainer, fp8_weights

pytestmark, SENT = pytest.mark.gpu, 0xA5
SHAPES = {"small": (64, 64), "one_chunk": (64, WQ_CHUNK // 64), "gap": (8, 128), "chunk_plus_8": (WQ_CHUNK // 8 + 1, 8),
          "several": (200, 128), "zero": (32, 64), "amax_1.75": (16, 64), "amax_above_1.75": (16, 64)}
COVERED = [k for k in SHAPES if k != "gap"]  # "gap": an uncovered slot of the source arena between covered ones


def _case(cuda):  # huge values in the gap and behind every tensor, 64 spare bytes between destinations, stale amax words
    g = torch.Generator().manual_seed(5)
    segs, parts, off = [], [], 0
    for name, (r, c) in SHAPES.items():
        x = torch.randn(r * c, generator=g) * {"gap": float("inf"), "zero": 0.0}.get(name, 1.0)
        if name == "several":
            x[-3] = -100.0  # the largest |x|, negative, in the tensor's last 16-B vector
        elif name.startswith("amax"):
            x = x.clamp(-1.5, 1.5)
            x[77] = 1.75 if name == "amax_1.75" else -(1.75 + 2.0 ** -7)  # m = 1.75 → e = 8; the next bf16 → e = 7
        parts += [x, torch.full((-r * c % 1024,), 3e38)]
        segs += [(off, r * c)] if name != "gap" else []
        off += r * c + -r * c % 1024
    rows, chunks, _ = wq_table(segs)
    rows = [(ch, src, dst + 64 * t, n) for t, (ch, src, dst, n) in enumerate(rows)]
    out = (torch.full((rows[-1][2] + rows[-1][3] + 64,), SENT, dtype=torch.uint8, device=cuda),
           torch.full((len(rows),), 0x7F7F0000, dtype=torch.int32, device=cuda), torch.zeros(len(rows), device=cuda))
    return torch.cat(parts).bfloat16(), rows, out, chunks


@pytest.fixture(scope="module")
def grouped(cuda):
    src, rows, first, chunks = _case(cuda)
    m = _native.require_hip()
    host, params = torch.tensor(rows, dtype=torch.int64), src.to(cuda)
    m.quant_e4m3_grouped(params, *first, host.to(cuda), host, chunks)
    _, so, _, n = rows[COVERED.index("several")]
    params[so:so + n] *= 2.0 ** -4  # exact in bf16
    again = tuple(t.clone() for t in first)  # the second run finds the first one's bytes and amax words
    m.quant_e4m3_grouped(params, *again, host.to(cuda), host, chunks)
    return src, rows, first, again


@pytest.mark.parametrize("t,name", enumerate(COVERED))
def test_grouped_bytes_and_scale_are_the_reference(grouped, t, name):
    src, rows, (q, amax, d), _ = grouped
    _, so, do, n = rows[t]
    x = src[so:so + n].view(SHAPES[name])
    q_ref, d_ref = ops.ref_quant_e4m3(x)
    assert torch.equal(d[t:t + 1].cpu(), d_ref) and int(amax[t]) == int(x.float().abs().max().view(torch.int32))
    bad = q[do:do + n].cpu() != q_ref.view(-1)
    assert not bad.any(), f"{int(bad.sum())} of {n} bytes differ, first at {int(bad.nonzero()[0])}"


def test_grouped_writes_nothing_else_and_clears_its_words(grouped):
    src, rows, (q, _, d), (q2, _, d2) = grouped
    want = torch.full_like(q, SENT).cpu()
    for _, so, do, n in rows:
        want[do:do + n] = ops.ref_quant_e4m3(src[so:so + n])[0]
    assert torch.equal(q.cpu(), want)  # bytes outside every destination keep the sentinel
    assert d[COVERED.index("amax_above_1.75")] == 2 * d[COVERED.index("amax_1.75")] == 2.0 ** -7  # both sides of the rule
    moved = torch.tensor([2.0 ** -4 if k == "several" else 1.0 for k in COVERED], device=d.device)
    assert torch.equal(d2, d * moved) and torch.equal(q2, q)  # a tensor × 2⁻⁴: its scale follows (cleared amax), bytes stay


@pytest.mark.parametrize("what", ["host_table_is_no_mirror", "offset_not_a_multiple_of_8", "wrong_chunk_total"])
def test_grouped_rejections(cuda, what):
    src, rows, out, chunks = _case(cuda)
    dev = torch.tensor(rows, dtype=torch.int64)
    host = dev[:-1].contiguous() if what == "host_table_is_no_mirror" else dev.clone()
    host[2, 1] += 4 * (what == "offset_not_a_multiple_of_8")
    with pytest.raises(RuntimeError):
        _native.require_hip().quant_e4m3_grouped(src.to(cuda), *out, dev.to(cuda), host, chunks + (what == "wrong_chunk_total"))
    assert bool((out[0] == SENT).all())  # nothing was launched


def _train(cuda, monkeypatch, fp8, K, hook):
    seen, live_wq = [], fp8_ops._live_wq
    cfg = GPT2Config.named("gpt2-smoke")
    cfg.fp8 = fp8
    tr = GPT2Trainer(cfg, 2, 256, cuda, seed=0, grad_accum=K)
    with monkeypatch.context() as mp:
        mp.setattr(fp8_ops, "_WQ_ARENA", [hook])
        mp.setattr(fp8_ops, "_live_wq", lambda w: seen.append(live_wq(w)) or seen[-1])
        losses = torch.stack([tr.step().detach() for _ in range(3)])
    return tr, losses, sum(r is not None for r in seen)  # how often a forward took a weight's arena copy


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("fp8", ["qkv", "ln", "lnmx"])
def test_trainer_is_bit_identical_with_the_arena_copies(cuda, monkeypatch, fp8, K):
    m = _native.require_hip()
    off, losses_off, hits_off = _train(cuda, monkeypatch, fp8, K, False)
    on, losses_on, hits_on = _train(cuda, monkeypatch, fp8, K, True)
    ws = fp8_weights(on.model, fp8)
    assert hits_off == 0 and hits_on == 3 * K * len(ws) and len(ws) == 2 * {"qkv": 1, "ln": 2, "lnmx": 3}[fp8]  # every product
    assert torch.equal(losses_on, losses_off) and torch.equal(on.flat.params, off.flat.params)
    with on.flat.wt_scope():  # staleness: the copies are those of the weights after the third optimizer step
        for w in ws:
            (q, d), (q_jit, d_jit) = fp8_ops._live_wq(w), m.quant_e4m3(w)
            assert torch.equal(q, q_jit) and torch.equal(d, d_jit)
    q, d = fp8_ops._weight_e4m3(ws[0])  # outside the scope: just in time
    assert q.data_ptr() != ws[0]._pdo_wq[1].data_ptr() and torch.equal(q, m.quant_e4m3(ws[0])[0])
    on.close(), off.close()
