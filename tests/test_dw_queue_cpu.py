"""The grouped weight-gradient queue (ops.core deferred_weight_grads) without a GPU: the flush rule
and the remainder rule as pure functions, and the queue's bookkeeping against a fake native module
(which launches nothing and records the calls)."""
import pytest
import torch

from paddle_operator_amd import _native
from paddle_operator_amd.ops import core

BF16 = torch.bfloat16
MEDIUM = (48, 16, 64, 64)  # GPT-2-medium's dW tiles per layer: qkv, proj, fc1, fc2
BIG = 1 << 60


def test_tiles():
    assert [core.dw_tiles(3072, 1024), core.dw_tiles(1024, 1024), core.dw_tiles(4096, 1024),
            core.dw_tiles(1024, 4096)] == list(MEDIUM)
    assert core.dw_tiles(640, 512) == 6  # a half-height last row counts as a tile row


def test_flush_rule_whole_rounds():
    assert not core.dw_should_flush([], 0, 256, BIG)
    assert not core.dw_should_flush([48, 16, 64], 0, 256, BIG)
    assert not core.dw_should_flush([255] * 3, 0, 256, BIG)
    assert core.dw_should_flush([256] * 3, 0, 256, BIG)
    assert core.dw_should_flush([64] * 12, 0, 256, BIG)
    assert not core.dw_should_flush([64] * 4, 0, 256, BIG)        # one round: below the group's 3 rounds
    assert core.dw_should_flush([64] * 4, 0, 256, BIG, min_rounds=1)
    assert core.dw_should_flush([8, 8], 0, 16, BIG, min_rounds=1)  # another CU count


@pytest.mark.parametrize("order", [MEDIUM, (64, 64, 16, 48)])  # as listed, and in the backward's order
def test_gpt2_medium_flushes_after_every_fourth_layer(order):
    q, flushed_after = [], []
    for layer in range(24):
        for i, t in enumerate(order):
            q.append(t)
            if core.dw_should_flush(q, 0, 256, BIG):
                flushed_after.append((layer, i))
                q = []
    assert flushed_after == [(l, 3) for l in (3, 7, 11, 15, 19, 23)]
    assert q == []


def test_byte_cap_forces_early_flush():
    assert not core.dw_should_flush([48], 100, 256, 100)
    assert core.dw_should_flush([48], 101, 256, 100)


def test_remainder_takes_the_split_path_below_the_fill_threshold():
    assert core.dw_grouped_prefix([], 256) == 0
    assert core.dw_grouped_prefix(list(MEDIUM), 256) == 0                  # 192 of 256 = 75 %
    assert core.dw_grouped_prefix(list(MEDIUM) + [48], 256) == 0           # 240 of 256 = 93.75 %
    assert core.dw_grouped_prefix(list(MEDIUM) + [48, 16], 256) == 6       # a full round
    assert core.dw_grouped_prefix(list(MEDIUM) * 4, 256) == 16             # three full rounds
    # four layers and one more GEMM: the whole rounds run grouped, the 17th entry alone
    assert core.dw_grouped_prefix(list(MEDIUM) * 4 + [64], 256) == 16
    assert core.dw_grouped_prefix([241], 256) == 1                         # 94.1 %
    assert core.dw_grouped_prefix([240], 256) == 0                         # 93.75 %
    assert core.dw_grouped_prefix([3, 1, 4, 4], 12) == 4                   # exactly one round of 12


class FakeT:
    """What the queue looks at of a GPU tensor."""
    is_cuda = True
    device = "fake"

    def __init__(self, *shape, dtype=BF16):
        self.shape, self.dtype = tuple(shape), dtype

    def is_contiguous(self):
        return True

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def view(self, *shape):
        return FakeT(*shape, dtype=self.dtype)


class FakeParam:
    _pdo_direct = True

    def __init__(self, name, M, N, log):
        self.name, self.grad, self.log = name, FakeT(M, N), log

    def _pdo_ready(self, p):
        assert p is self
        self.log.append(("ready", self.name))


class FakeNative:
    def __init__(self, log):
        self.log = log

    def gemm_dw_grouped_ok(self, T, M, N):
        return M % 128 == 0 and N % 256 == 0 and T % 128 == 0 and T >= 256

    def gemm_dw_grouped(self, dys, xs, outs, accs):
        assert len(dys) == len(xs) == len(outs) == len(accs) and all(accs)
        self.log.append(("grouped", [(d.shape[1], x.shape[1]) for d, x in zip(dys, xs)]))
        return True

    def gemm_dw(self, dy, x, out, acc, splits=0):
        self.log.append(("single", (dy.shape[1], x.shape[1])))
        return True


@pytest.fixture
def fake(monkeypatch):
    log = []
    monkeypatch.setattr(_native, "require_hip", lambda: FakeNative(log))
    monkeypatch.setattr(_native, "ops_mode", lambda: "hip")
    monkeypatch.setattr(_native, "hip_ext", lambda: None)  # flush_deferred: no column sums here
    monkeypatch.setattr(core, "_DW_CUS", [8])
    monkeypatch.setattr(core, "_DW_GROUPED", [True])
    assert core._dw_queue.depth == 0 and not core._dw_queue.entries
    yield log
    assert core._dw_queue.depth == 0 and not core._dw_queue.entries


def _push(name, M, N, log, T=256):
    p = FakeParam(name, M, N, log)
    with torch.no_grad():
        assert core._weight_grad(p, FakeT(T, M), FakeT(T, N)) is None
    return p


def test_ready_fires_once_in_queue_order_after_the_flush(fake):
    log = fake
    with core.deferred_weight_grads("cuda"):
        _push("a", 1024, 1024, log)   # 16 tiles on 8 CUs: two rounds, below the group's three
        _push("b", 256, 512, log)     # 2 more: 18
        assert log == [] and len(core._dw_queue.entries) == 2
        _push("c", 768, 512, log)     # 6 more: 24 = three whole rounds -> flush
        assert log == [("grouped", [(1024, 1024), (256, 512), (768, 512)]),
                       ("ready", "a"), ("ready", "b"), ("ready", "c")]
        assert not core._dw_queue.entries
        _push("d", 512, 1024, log)    # 8 tiles: one whole round, held for the exit
        _push("e", 256, 256, log)     # 1 tile: a remainder of 12.5 %
        assert len(log) == 4
    assert log[4:] == [("grouped", [(512, 1024)]), ("single", (256, 256)), ("ready", "d"), ("ready", "e")]


def test_outside_the_scope_and_with_the_hook_off_nothing_is_queued(fake, monkeypatch):
    log = fake
    _push("a", 256, 256, log)
    assert log == [("single", (256, 256)), ("ready", "a")]
    del log[:]
    monkeypatch.setattr(core, "_DW_GROUPED", [False])
    with core.deferred_weight_grads("cuda"):
        _push("b", 256, 256, log)
        assert log == [("single", (256, 256)), ("ready", "b")]


def test_out_of_contract_shape_is_not_queued(fake):
    log = fake
    with core.deferred_weight_grads("cuda"):
        _push("a", 256, 256, log, T=192)
        assert log == [("single", (256, 256)), ("ready", "a")]


def test_flush_deferred_flushes_the_queue(fake):
    log = fake
    with core.deferred_weight_grads("cuda"):
        _push("a", 512, 1024, log)
        assert log == []
        core.flush_deferred()
        assert log == [("grouped", [(512, 1024)]), ("ready", "a")]
    assert len(log) == 2


def test_byte_cap_flushes_in_the_queue(fake, monkeypatch):
    log = fake
    monkeypatch.setattr(core, "_DW_CAP_BYTES", [(256 * 512 + 256 * 1024) * 2 - 1])
    with core.deferred_weight_grads("cuda"):
        _push("a", 512, 1024, log)
        assert log == [("grouped", [(512, 1024)]), ("ready", "a")]


def test_a_ready_hook_that_flushes_again_sees_an_empty_queue(fake):
    log = fake
    with core.deferred_weight_grads("cuda"):
        p = _push("a", 512, 1024, log)
        p._pdo_ready = lambda q: (core.flush_deferred(), log.append(("ready", "a")))
        core.flush_weight_grads()
    assert log == [("grouped", [(512, 1024)]), ("ready", "a")]
