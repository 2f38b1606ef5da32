"""CPU self-checks of the float64 references that test_small_kernels_gpu.py holds the HIP kernels to."""
import math

import torch

from test_small_kernels_gpu import (_bucket_layout, _chunk_sums, _halfway_f32, _transpose_table, adamw_ref, clip_coef,
                                    f32, sgd_ref, xent_ref)


def test_adamw_reference_matches_torch_adamw_fp64():
    """Three steps of the textbook formula vs torch.optim.AdamW in float64, one parameter group with weight
    decay and one without, grad_scale and the clip coefficient applied to the gradient beforehand."""
    g = torch.Generator().manual_seed(0)
    lr, b1, b2, eps, wd = 3e-4, 0.9, 0.95, 1e-8, 0.1
    n = 4096
    w0 = 0.02 * torch.randn(2, n, generator=g, dtype=torch.float64)
    pa, pb = (torch.nn.Parameter(w0[i].clone()) for i in range(2))
    opt = torch.optim.AdamW([{"params": [pa], "weight_decay": wd}, {"params": [pb], "weight_decay": 0.0}], lr=lr,
                            betas=(b1, b2), eps=eps)
    w = w0.clone()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    dec = torch.tensor([[1.0], [0.0]], dtype=torch.float64)
    for t, (normsq, clip) in enumerate([(4.0, 1.0), (0.25, 1.0), (math.nan, -1.0)], start=1):
        grad = torch.randn(2, n, generator=g, dtype=torch.float64)
        grad[:, ::17] = 0.0
        c = clip_coef(normsq, clip, 0.25)
        pa.grad, pb.grad = c * grad[0], c * grad[1]
        opt.step()
        w, m, v, _ = adamw_ref(w, m, v, grad, dec, c, lr, b1, b2, eps, wd, 1.0 - b1 ** t, 1.0 - b2 ** t)
        for got, want in ((w[0], pa.detach()), (w[1], pb.detach())):
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        st = opt.state[pa]
        assert float((m[0] - st["exp_avg"]).abs().max()) <= 1e-12 * float(st["exp_avg"].abs().max())
        assert float((v[0] - st["exp_avg_sq"]).abs().max()) <= 1e-12 * float(st["exp_avg_sq"].abs().max())


def test_clip_coef_modes():
    assert clip_coef(4.0, 1.0, 0.25) == 0.25 / (2.0 + 1e-6)
    assert clip_coef(0.25, 1.0, 0.25) == 0.25
    assert clip_coef(math.nan, -1.0, 0.25) == 0.25


def test_sgd_reference_matches_torch_sgd_fp64():
    g = torch.Generator().manual_seed(1)
    lr, mom, wd = 0.1, 0.9, 1e-4
    w0 = torch.randn(2, 512, generator=g, dtype=torch.float64)
    pa, pb = (torch.nn.Parameter(w0[i].clone()) for i in range(2))
    opt = torch.optim.SGD([{"params": [pa], "weight_decay": wd}, {"params": [pb], "weight_decay": 0.0}], lr=lr,
                          momentum=mom)
    w, buf = w0.clone(), torch.zeros_like(w0)
    dec = torch.tensor([[1.0], [0.0]], dtype=torch.float64)
    for _ in range(3):
        grad = torch.randn(2, 512, generator=g, dtype=torch.float64)
        pa.grad, pb.grad = 0.25 * grad[0], 0.25 * grad[1]
        opt.step()
        w, buf = sgd_ref(w, buf, grad, dec, lr, mom, wd, 0.25)
        assert float((w[0] - pa.detach()).abs().max()) <= 1e-12 * float(pa.detach().abs().max())
        assert float((w[1] - pb.detach()).abs().max()) <= 1e-12 * float(pb.detach().abs().max())


def test_xent_reference_matches_torch_cross_entropy():
    g = torch.Generator().manual_seed(2)
    V, Vp = 21, 24
    tgt = torch.tensor([0, V - 1, 10, -100, 22, 3])
    lg = (2.0 * torch.randn(6, Vp, generator=g)).bfloat16()
    lg[:, V:] = 100.0
    x = lg[:, :V].double().requires_grad_()
    t = torch.where(tgt < V, tgt, torch.full_like(tgt, -100))  # a target in the padding counts as ignored
    want = torch.nn.functional.cross_entropy(x, t, ignore_index=-100)
    (0.5 * want).backward()
    loss, lse, d, cnt = xent_ref(lg, tgt, V, 0.5)
    assert cnt == 4 and abs(loss - float(want.detach())) <= 1e-12
    assert float((d[:, :V] - x.grad).abs().max()) <= 1e-15
    assert float(d[:, V:].abs().max()) == 0.0 and float(d[3].abs().max()) == 0.0 and float(d[4].abs().max()) == 0.0
    assert float((lse - torch.logsumexp(x.detach(), 1)).abs().max()) == 0.0
    loss, _, d, cnt = xent_ref(lg[:3], torch.tensor([-100, 22, -100]), V)
    assert loss == 0.0 and cnt == 0 and float(d.abs().max()) == 0.0


def test_f32_helper_rounds_to_float32():
    assert f32(0.9) == 0.89999997615814208984375
    assert 1.0 - f32(0.9) == float(torch.tensor(1.0) - torch.tensor(0.9))  # 1 − b1 is exact in fp32


def test_bucket_layout_has_the_edges():
    sizes, offsets, total = _bucket_layout()
    assert len(sizes) == 106 and offsets[0] == 24 and sizes[50] == 0
    assert all(n % 2 == 1 for i, n in enumerate(sizes) if i != 50)
    ends = [o + n for o, n in zip(offsets, sizes)]
    assert all(offsets[i + 1] >= ends[i] for i in range(105)) and total > ends[-1]
    lo = offsets[60] - 24 - 2048  # a whole 2048-element span that no tensor touches
    assert lo % 2048 == 0 and ends[59] <= lo
    assert any(o // 2048 != (o + n - 1) // 2048 for o, n in zip(offsets, sizes) if n)
    assert offsets[80] % 2048 == 2043 and sizes[80] > 5


def test_chunk_sums_pads_the_short_last_chunk():
    g = torch.arange(20, dtype=torch.float32).bfloat16()
    want = [float(sum(i * i for i in range(a, min(a + 8, 20)))) for a in (0, 8, 16)]
    assert _chunk_sums(g, 8).tolist() == want


def test_halfway_values_are_ties_and_their_neighbours():
    x = _halfway_f32(torch.device("cpu"), 4096, torch.Generator().manual_seed(3))
    low = x.view(torch.int32) & 0xFFFF
    assert set(low.tolist()) == {0x7FFF, 0x8000, 0x8001}
    assert bool(torch.isfinite(x).all()) and bool((x < 0).any()) and bool((x > 0).any())
    up = (x.view(torch.int32) >> 16) & 1
    tie = low == 0x8000
    assert bool((up[tie] == 0).any()) and bool((up[tie] == 1).any())  # even and odd lower neighbours
    # round-to-nearest-even on the integer pattern
    b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    want = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    got = x.bfloat16().view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(got, want)


def test_transpose_table_is_disjoint_and_aligned():
    rows, tiles, nsrc, ndst = _transpose_table()
    assert tiles == sum((r[3] // 64) * (r[4] // 64) for r in rows) == 1 + 3 + 10 + 2
    for a, b in zip(rows, rows[1:]):
        assert b[1] >= a[1] + a[3] * a[4] + 1024 and b[2] >= a[2] + a[3] * a[4] + 1024
    assert all(r[1] % 1024 == 0 and r[2] % 1024 == 0 for r in rows)
    assert rows[-1][1] + rows[-1][3] * rows[-1][4] <= nsrc and rows[-1][2] + rows[-1][3] * rows[-1][4] <= ndst
