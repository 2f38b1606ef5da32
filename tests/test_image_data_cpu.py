"""Image files on the CPU: the crop sampler's invariants, the evaluation stream's coverage, the
host reference of the resample at its exact points, the format checks, the shared learning-rate
formula, and the tiny ResNet trainer end to end (evaluate, checkpoint and resume) on ``.npy`` sets
written under ``tmp_path``.
"""
import math

import numpy as np
import pytest
import torch

from paddle_operator_amd import data as D
from paddle_operator_amd.ops.optim import cosine_lr

SEED = 0xF234_5678_9ABC_DEF1


def _write_set(path, n, R, classes, seed=0, labels_dtype=np.int64):
    rng = np.random.default_rng(seed)
    path.mkdir(parents=True, exist_ok=True)
    img = rng.integers(0, 256, (n, R, R, 3), dtype=np.uint8)
    lab = rng.integers(0, classes, n).astype(labels_dtype)
    np.save(path / "images.npy", img)
    np.save(path / "labels.npy", lab)
    return img, lab


# ----------------------------------------------------------------------------- crop_boxes
@pytest.mark.parametrize("R,res", [(36, 32), (40, 32), (256, 224)])
def test_crop_boxes_invariants(R, res):
    B, n = 1000, 12345
    bx = np.concatenate([D.crop_boxes(SEED, 0, m, 0, B, n, R, res) for m in range(100)])  # 10^5 draws
    i, x0, y0, cw, ch, flip = bx.T
    assert i.min() >= 0 and i.max() < n and set(np.unique(flip)) == {0, 1}
    assert cw.min() >= 1 and ch.min() >= 1 and cw.max() <= R and ch.max() <= R
    assert x0.min() >= 0 and y0.min() >= 0 and (x0 + cw <= R).all() and (y0 + ch <= R).all()
    # area: the drawn sides are floors of a = s·√r and b = s/√r with a·b = f·R², f in [0.08, 1):
    # (cw + 1)(ch + 1) > 0.08·R² where nothing was clamped up to 1, and cw·ch ≤ R² always
    area = cw * ch
    assert (area <= R * R).all()
    free = (cw < R) & (ch < R)
    assert ((cw + 1) * (ch + 1) >= 0.08 * R * R)[free].all()
    # ratio within one pixel of [3/4, 4/3] where neither side was clamped: the long side over
    # the short side is r = t² in [1, 4/3) before the floors, so hi ≤ a ≤ 4/3·b < 4/3·(lo + 1)
    lo, hi = np.minimum(cw, ch), np.maximum(cw, ch)
    assert (hi[free] * 3 < (lo[free] + 1) * 4).all()
    # both orientations and a spread of positions occur
    assert (cw > ch).any() and (ch > cw).any() and x0.max() > 0 and y0.max() > 0


def test_global_batch_depends_on_seed_and_m_only():
    B, n, R, res = 5, 999, 40, 32
    for m in (0, 7, 2**32 - 1):
        whole = D.crop_boxes(SEED, 0, m, 0, 2 * B, n, R, res)
        halves = np.concatenate([D.crop_boxes(SEED, 0, m, r, B, n, R, res) for r in (0, 1)])
        assert np.array_equal(whole, halves)
    assert not np.array_equal(D.crop_boxes(SEED, 0, 0, 0, B, n, R, res), D.crop_boxes(SEED, 0, 1, 0, B, n, R, res))
    assert not np.array_equal(D.crop_boxes(SEED, 0, 0, 0, B, n, R, res), D.crop_boxes(SEED + 1, 0, 0, 0, B, n, R, res))
    assert np.array_equal(D.crop_boxes(SEED, 0, 2**32 + 3, 0, B, n, R, res), D.crop_boxes(SEED, 0, 3, 0, B, n, R, res))


@pytest.mark.parametrize("world", [1, 2])
def test_evaluation_stream_visits_every_image_once(world):
    n, B, R, res = 11, 4, 40, 32
    Bg = world * B
    seen, pads = [], 0
    for m in range(-(-n // Bg)):
        for rank in range(world):
            bx = D.crop_boxes(SEED, 1, m, rank, B, n, R, res, Bg)
            assert (bx[:, 1:] == [(R - res) // 2, (R - res) // 2, res, res, 0]).all()
            seen += [int(i) for i in bx[:, 0] if i >= 0]
            pads += int((bx[:, 0] < 0).sum())
    assert sorted(seen) == list(range(n)) and pads == -(-n // Bg) * Bg - n
    # padding rows: label −1 and a zero image
    img = np.random.default_rng(0).integers(0, 256, (n, R, R, 3), dtype=np.uint8)
    lab = np.arange(n) % 7
    bx = D.crop_boxes(SEED, 1, -(-n // Bg) - 1, world - 1, B, n, R, res, Bg)
    x, y = D.image_batch_ref(img, lab, bx, res, *D.image_norm())
    for j in range(B):
        if bx[j, 0] < 0:
            assert y[j] == -1 and not x[j].float().any()
        else:
            assert y[j] == lab[bx[j, 0]]


# ----------------------------------------------------------------------------- image_batch_ref
def test_reference_is_a_copy_at_the_crop_size():
    R, res, n = 40, 32, 3
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (n, R, R, 3), dtype=np.uint8)
    lab = np.array([4, 5, 6])
    boxes = np.array([[2, 3, 5, res, res, 0], [0, 8, 0, res, res, 1], [1, 0, 8, res, res, 0]], dtype=np.int64)
    x, y = D.image_batch_ref(img, lab, boxes, res, (1.0 / 65536,) * 3, (0.0,) * 3)
    assert x.dtype == torch.bfloat16 and tuple(x.shape) == (3, res, res, 3) and y.tolist() == [6, 4, 5]
    for j, (i, x0, y0, cw, ch, flip) in enumerate(boxes.tolist()):
        crop = img[i, y0:y0 + ch, x0:x0 + cw].astype(np.float32)  # 0 … 255: exact in bf16
        want = crop[:, ::-1] if flip else crop
        assert np.array_equal(x[j].float().numpy(), want), j
    # staged: row j reads entry j
    xs, ys = D.image_batch_ref(img[boxes[:, 0]], lab[boxes[:, 0]], boxes, res, (1.0 / 65536,) * 3, (0.0,) * 3,
                               staged=True)
    assert torch.equal(xs.view(torch.int16), x.view(torch.int16)) and torch.equal(ys, y)


def test_bf16_rounding_is_nearest_even():
    v = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 255.5, 3.0e-5], dtype=np.float32)
    got = torch.from_numpy(D.bf16_rne_bits(v)).view(torch.bfloat16)
    assert torch.equal(got, torch.from_numpy(v).to(torch.bfloat16))


def test_bf16_floor_ceil_helper_of_the_gpu_tests():
    from test_image_data_gpu import bf16_floor_ceil
    v = torch.tensor([1.0, 1.001, -1.001, 255.3, -0.3, 3.0e-5, 0.0, -1e-30, 1e-30], dtype=torch.float64)
    lo, hi = bf16_floor_ceil(v)
    for a in (lo, hi):
        assert torch.equal(a.to(torch.bfloat16).double(), a)  # representable
    assert bool((lo <= v).all() and (v <= hi).all() and ((hi - lo) <= v.abs() * 2.0 ** -7 + 1e-300).all())
    assert lo[0] == hi[0] == 1.0 and lo[6] == hi[6] == 0.0 and bool((lo[1:6] < hi[1:6]).all())


# ----------------------------------------------------------------------------- format checks
def test_format_rejections_name_the_file(tmp_path):
    good = tmp_path / "good"
    _write_set(good, 6, 40, 10, labels_dtype=np.uint8)
    images, labels = D.open_images(str(good), 32, 10)
    assert images.shape == (6, 40, 40, 3) and labels.shape == (6,)

    def bad(name, images=None, labels=None, res=32, classes=10, which="images.npy"):
        d = tmp_path / name
        img, lab = _write_set(d, 6, 40, 10)
        if images is not None:
            np.save(d / "images.npy", images(img))
        if labels is not None:
            np.save(d / "labels.npy", labels(lab))
        with pytest.raises(ValueError) as e:
            D.open_images(str(d), res, classes)
        assert str(d / which) in str(e.value), str(e.value)

    bad("dtype", images=lambda a: a.astype(np.int16))
    bad("rank", images=lambda a: a[..., 0])
    bad("channels", images=lambda a: np.concatenate([a, a[..., :1]], axis=3))
    bad("square", images=lambda a: a[:, :, :36])
    bad("small", res=48)
    bad("res8", res=36)
    bad("float-labels", labels=lambda l: l.astype(np.float32), which="labels.npy")
    bad("label-range", classes=5, labels=lambda l: np.full_like(l, 5), which="labels.npy")
    bad("negative-label", labels=lambda l: l - 100, which="labels.npy")
    bad("label-count", labels=lambda l: l[:-1], which="labels.npy")
    bad("label-rank", labels=lambda l: l.reshape(2, 3), which="labels.npy")


# ----------------------------------------------------------------------------- the schedule
def _cosine_inline(step, base_lr, warmup, total, min_ratio):
    """The formula as the GPT-2 trainer first carried it."""
    if step < warmup:
        return base_lr * (step + 1) / warmup
    p = min(1.0, (step - warmup) / max(1, total - warmup))
    return base_lr * (min_ratio + (1 - min_ratio) * 0.5 * (1 + math.cos(math.pi * p)))


def test_shared_cosine_is_the_gpt2_trainers_curve():
    from paddle_operator_amd.models.gpt2 import GPT2Config
    from paddle_operator_amd.train import GPT2Trainer
    from paddle_operator_amd.workloads.resnet import ResNetTrainer
    kw = dict(lr_schedule="cosine", lr_warmup=3, lr_decay_steps=9, lr_min_ratio=0.05)
    g = GPT2Trainer(GPT2Config.named("gpt2-tiny"), 2, 32, "cpu", dtype=torch.float32, lr=6e-4, **kw)
    r = ResNetTrainer(2, "cpu", tiny=True, lr=0.4, **kw)
    for s in range(12):
        g.opt.step_count = r.opt.step_count = s
        assert g.next_lr() == cosine_lr(s, 6e-4, 3, 9, 0.05) == _cosine_inline(s, 6e-4, 3, 9, 0.05)
        assert r.next_lr() == cosine_lr(s, 0.4, 3, 9, 0.05) == _cosine_inline(s, 0.4, 3, 9, 0.05)
    assert ResNetTrainer(2, "cpu", tiny=True).lr_dev is None  # no schedule: lr by value, as before
    with pytest.raises(ValueError):
        ResNetTrainer(2, "cpu", tiny=True, lr_schedule="linear")


# ----------------------------------------------------------------------------- the tiny trainer
@pytest.fixture
def sets(tmp_path):
    _write_set(tmp_path / "train", 24, 40, 10, seed=1)
    _write_set(tmp_path / "val", 11, 36, 10, seed=2, labels_dtype=np.uint8)
    return str(tmp_path / "train"), str(tmp_path / "val")


def _trainer(sets, **kw):
    from paddle_operator_amd.workloads.resnet import ResNetTrainer
    torch.manual_seed(0)
    return ResNetTrainer(4, "cpu", tiny=True, data=sets[0], val_data=sets[1], data_seed=SEED, lr=0.05, **kw)


def test_trainer_draws_the_reference_batches(sets):
    tr = _trainer(sets)
    assert tr.data.placement == tr.val.placement == "cpu" and tr.classes == 10
    for s in range(2):
        x, y = tr.batch()
        wx, wy = tr.data.host_batch(s)
        assert torch.equal(y, wy) and torch.equal(x, wx.permute(0, 3, 1, 2).float())
        tr.opt.step_count += 1


def test_evaluate_counts_every_image_and_matches_a_recount(sets):
    tr = _trainer(sets)
    tr.step()
    stats = {k: v.clone() for k, v in tr.model.named_buffers()}
    params, step = tr.flat.params.clone(), tr.opt.step_count
    ev = tr.evaluate()
    assert ev["images"] == 11 and set(ev) == {"val_loss", "top1", "top5", "images"}
    assert ev == tr.evaluate() and tr.model.training and tr.opt.step_count == step
    assert torch.equal(tr.flat.params, params)
    assert all(torch.equal(v, stats[k]) for k, v in tr.model.named_buffers())
    # plain torch on the stored centre crops
    img, lab = np.load(sets[1] + "/images.npy"), np.load(sets[1] + "/labels.npy").astype(np.int64)
    sc, sh = D.image_norm()
    c = img[:, 2:34, 2:34].astype(np.float32) * np.float32(65536.0)
    x = torch.from_numpy(c * np.asarray(sc, np.float32) + np.asarray(sh, np.float32)).to(torch.bfloat16).float()
    tr.model.eval()
    with torch.no_grad():
        out = tr.model(x.permute(0, 3, 1, 2).contiguous())
    tr.model.train()
    y = torch.from_numpy(lab)
    top5 = out.topk(5, dim=1).indices
    assert ev["top1"] == float((out.argmax(1) == y).sum()) / 11
    assert ev["top5"] == float((top5 == y[:, None]).any(1).sum()) / 11
    assert abs(ev["val_loss"] - float(torch.nn.functional.cross_entropy(out, y))) < 1e-5
    assert tr.evaluate(1)["images"] == 4
    from paddle_operator_amd.workloads.resnet import ResNetTrainer
    with pytest.raises(RuntimeError):
        ResNetTrainer(4, "cpu", tiny=True).evaluate()


def test_resume_replays_batches_and_losses(sets):
    kw = dict(lr_schedule="cosine", lr_warmup=2, lr_decay_steps=6)
    a = _trainer(sets, **kw)
    for _ in range(2):
        a.step()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    sd["buffers"] = {k: v.clone() for k, v in sd["buffers"].items()}
    assert sd["step"] == 2
    b = _trainer(sets, **kw)
    b.load_state_dict(sd)
    assert b.opt.step_count == 2
    for s in range(2, 5):
        xa, ya = a.batch()
        xb, yb = b.batch()
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
        la, lb = a.step(), b.step()
        assert float(la) == float(lb) and float(a.lr_dev) == float(b.lr_dev) == float(np.float32(
            cosine_lr(s, 0.05, 2, 6, 0.1)))
    assert torch.equal(a.flat.params, b.flat.params) and torch.equal(a.opt.buf, b.opt.buf)
    # a checkpoint from before "step" existed still loads (and starts the stream at 0)
    old = {k: v for k, v in sd.items() if k != "step"}
    c = _trainer(sets, **kw)
    c.load_state_dict(old)
    assert c.opt.step_count == 0 and torch.equal(c.flat.params, sd["params"])


def test_parse_args_resnet_flags():
    from paddle_operator_amd.launch.run import _resnet_flags, parse_args
    a = parse_args(["--workload", "resnet50", "--data", "d", "--val-data", "v", "--data-seed", "7",
                    "--data-device-gb", "0.5", "--lr-schedule", "cosine", "--lr-warmup", "5", "--lr-decay-steps", "90",
                    "--lr-min-ratio", "0.01", "--eval-every", "10"])
    assert (a.data, a.val_data, a.data_seed, a.data_device_gb) == ("d", "v", 7, 0.5)
    assert (a.lr_schedule, a.lr_warmup, a.lr_decay_steps, a.lr_min_ratio) == ("cosine", 5, 90, 0.01)
    assert a.lr == 0.1 and a.eval_every == 10 and a.eval_batches == 0
    assert _resnet_flags(a) == {"data": "d", "lr_schedule": "cosine"}
    assert parse_args(["--workload", "gpt2"]).lr == 3e-4 and parse_args(["--workload", "gpt2"]).eval_batches == 8
    b = parse_args(["--workload", "resnet50", "--lr", "0.4", "--eval-batches", "3"])
    assert b.lr == 0.4 and b.eval_batches == 3 and _resnet_flags(b) == {"lr": 0.4}
    assert parse_args(["--workload", "gpt2", "--lr", "1e-3"]).lr == 1e-3
    assert _resnet_flags(parse_args(["--workload", "resnet50"])) == {}
