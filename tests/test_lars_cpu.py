"""FlatLARS's torch path against a per-parameter float64 loop of the rule; the launcher's flag."""
import pytest
import torch


def test_flat_lars_torch_path_matches_fp64_loop():
    from paddle_operator_amd.models.resnet import resnet18_like_tiny
    from paddle_operator_amd.parallel.flat import FlatParams
    from paddle_operator_amd.workloads.resnet import FlatLARS

    torch.manual_seed(0)
    flat = FlatParams(resnet18_like_tiny(10), dtype=torch.float32, device="cpu")
    lr, mom, wd, coeff, eps, sc = 0.2, 0.9, 1e-3, 0.01, 1e-9, 0.5
    opt = FlatLARS(flat, lr=lr, momentum=mom, weight_decay=wd, coeff=coeff, eps=eps)
    ref = {s.name: (s.param.detach().double().clone(), torch.zeros(s.shape, dtype=torch.float64)) for s in flat.slots}
    for _ in range(3):
        for s in flat.slots:
            s.param.grad.copy_(torch.randn(s.shape))
        for s in flat.slots:
            w, v = ref[s.name]
            g = sc * s.param.grad.double()
            W, G = float(w.norm()), float(g.norm())
            lam = coeff * W / (G + wd * W + eps) if s.decay and W > 0 and G > 0 else 1.0
            v.mul_(mom).add_(lr * lam * (g + wd * float(s.decay) * w))
            w.sub_(v)
        opt.step(sc)
    for s in flat.slots:  # three fp32 steps against float64
        torch.testing.assert_close(s.param.detach().double(), ref[s.name][0], rtol=1e-5, atol=1e-6)
    assert opt.state_dict()["optimizer"] == "lars" and opt.state_dict()["step"] == 3


def test_launcher_rejects_lars_outside_resnet(capsys):
    from paddle_operator_amd.launch.run import parse_args
    assert parse_args(["--workload", "resnet50", "--optimizer", "lars", "--lars-coeff", "0.002"]).lars_coeff == 0.002
    with pytest.raises(SystemExit):
        parse_args(["--workload", "gpt2", "--optimizer", "lars"])
    assert "resnet50 only" in capsys.readouterr().err
