"""The grouped weight-gradient queue in the trainer's backward (ops.core deferred_weight_grads) on
gpt2-smoke (width 256, 2 layers, seq 512, batch 2: 12 dW tiles per layer).

One trainer backward with the queue on (``_DW_GROUPED``; ``_DW_CUS`` = 12, so the 24 queued tiles are
two whole rounds and run as one grouped launch) and off, both against the fp32 CPU model at the same
weights, beside the framework's own bf16 error (the bf16 model on plain torch ops, as
test_trainer_gpu.py computes it):

* every arena gradient within that test's bound, error <= 1.5 x framework-bf16 error + 0.005;
* grouped error <= ungrouped error + framework-bf16 error, per parameter;
* nothing is left queued after the scope, and the GEMMs did run grouped (or not, with the hook off);
* accumulation: GPT2Trainer(grad_accum=2) over the same micro-batch twice adds two halves — the same
  gradient, within the same bound.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B, S = 2, 512


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))


def _view(buf, s):
    return buf[s.offset:s.offset + s.numel].view(s.shape)


def _torch_grads(model, slots, master, x, y):
    """Gradients of ``model`` on plain torch ops at the weights ``master`` (fp32 arena layout)."""
    params = dict(model.named_parameters())
    with torch.no_grad():
        for s in slots:
            params[s.name].copy_(_view(master, s))
    model.zero_grad(set_to_none=True)
    os.environ["PDO_OPS"] = "torch"
    try:
        model(x, y).backward()
    finally:
        os.environ["PDO_OPS"] = "hip"
    return {n: p.grad.detach().float().cpu() for n, p in params.items()}


def _trainer(dev, **kw):
    from paddle_operator_amd.models.gpt2 import GPT2Config
    from paddle_operator_amd.train import GPT2Trainer
    return GPT2Trainer(GPT2Config.named("gpt2-smoke"), B, S, dev, **kw)


def _step_grads(tr, x, y):
    """tr.step (forward, the backward in its deferred scopes, drain, optimizer), then the arena's
    gradients, which stay as the backward left them until the next step."""
    from paddle_operator_amd.ops import core
    n0 = core._dw_queue.n_grouped
    tr.step(x, y)
    torch.cuda.synchronize()
    assert core._dw_queue.depth == 0 and not core._dw_queue.entries and core._dw_queue.held == 0, "left queued"
    g = {s.name: (_view(tr.flat.param_grads, s).float() * tr.ddp.grad_scale).cpu() for s in tr.flat.slots}
    return g, core._dw_queue.n_grouped - n0


@pytest.fixture(scope="module")
def runs(cuda):
    """(fp32 CPU gradients, framework-bf16 gradients, {mode: (arena gradients, problems run grouped)})."""
    from paddle_operator_amd.models.gpt2 import GPT2, GPT2Config
    from paddle_operator_amd.ops import core
    saved = core._DW_GROUPED[0], core._DW_CUS[0]
    os.environ["PDO_OPS"] = "hip"
    try:
        out, master0, xy = {}, None, None
        for mode in ("grouped", "single", "accum"):
            core._DW_GROUPED[0] = mode != "single"
            core._DW_CUS[0] = 12
            tr = _trainer(cuda, grad_accum=2 if mode == "accum" else 1)
            if master0 is None:
                master0 = tr.opt.master.clone()
                xy = tr.batch()
            assert torch.equal(tr.opt.master, master0), "the trainers must start from the same weights"
            x, y = xy
            if mode == "accum":
                x, y = torch.cat([x, x]), torch.cat([y, y])
            out[mode] = _step_grads(tr, x, y)
            slots = tr.flat.slots
            del tr
        cfg = GPT2Config.named("gpt2-smoke")
        ref = _torch_grads(GPT2(cfg), slots, master0.cpu(), xy[0].cpu(), xy[1].cpu())
        with torch.device(cuda):
            fw_model = GPT2(cfg).bfloat16()
        fw = _torch_grads(fw_model, slots, master0, xy[0], xy[1])
        return ref, fw, out
    finally:
        core._DW_GROUPED[0], core._DW_CUS[0] = saved


def test_the_queue_ran_grouped_and_the_hook_turns_it_off(runs):
    _, _, out = runs
    assert out["grouped"][1] == 8   # qkv, proj, fc1, fc2 of both layers in the exit flush
    assert out["single"][1] == 0
    assert out["accum"][1] == 16    # one flush per micro-batch


@pytest.mark.parametrize("mode", ["grouped", "single", "accum"])
def test_arena_gradients_within_the_fp32_anchor_bound(runs, mode):
    ref, fw, out = runs
    errs = {n: (_rel(g, ref[n]), _rel(fw[n], ref[n])) for n, g in out[mode][0].items()}
    print({n: (round(eh, 5), round(ef, 5)) for n, (eh, ef) in errs.items()})
    bad = {n: (round(eh, 4), round(ef, 4)) for n, (eh, ef) in errs.items() if not eh <= 1.5 * ef + 0.005}
    assert not bad, bad


def test_grouped_error_not_above_ungrouped_plus_framework_error(runs):
    ref, fw, out = runs
    bad = {}
    for n in ref:
        eg, es, ef = _rel(out["grouped"][0][n], ref[n]), _rel(out["single"][0][n], ref[n]), _rel(fw[n], ref[n])
        if not eg <= es + ef:
            bad[n] = (eg, es, ef)
    assert not bad, bad
