"""Inference BatchNorm on the MI355X (batchnorm.hip bn_eval_ss + the apply kernels): bn_act_eval, its
pair form and bn_relu_pool_eval against float64 from the running statistics, and the full-width
ResNet-50 in eval mode on the hand-written kernels against fp32.

Bound of the per-element checks.  The float64 value is v = (x − mean)·γ / √(var + eps) + β (+ the
residual term), ReLU.  The kernels evaluate it in fp32 as x·sc + sh with sc = γ·rsqrt(var + eps),
sh = β − mean·sc (u = 2⁻²⁴, first order, the model of test_bn_kernels_gpu.py):
    invstd: the add var + eps (u/2 relative after the root) + 2u for rsqrtf      e_inv = 2.5u·invstd
    sc = γ·invstd                                                               e_sc  = |γ|·e_inv + u·|sc|
    sh = β − mean·sc                                       e_sh  = |mean|·e_sc + u·|mean·sc| + u·|sh|
    v = x·sc + sh                                          e_v   = |x|·e_sc + e_sh + u·|x·sc| + u·|v|
    + residual r (fp32 add), or + (r·rsc + rsh) with its own e_v                + u·|v + r|
and round once to bf16, so an output lies between the bf16 below v − e_v and the bf16 above
v + e_v.  Wherever e_v is far below the bf16 spacing at v — everywhere but at cancellation — these
are the two bf16 neighbours of v; the number of outputs outside the plain two neighbours is
printed and bounded by the share of elements with |v| < 2⁹·e_v.
"""
import copy
import os

import numpy as np
import pytest
import torch

from test_image_data_gpu import bf16_floor_ceil

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF16, F64 = torch.bfloat16, torch.float64
EPS = 1e-5


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def nhwc(rows, N, H, W):
    """[M, C] rows → the channels_last [N, C, H, W] view of the same memory."""
    return rows.reshape(N, H, W, rows.shape[1]).permute(0, 3, 1, 2)


def rows_of(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _bn(C, gen, cuda):
    """γ, β, running mean, running var (fp32, device) of one BatchNorm."""
    r = lambda lo, hi: (torch.rand(C, generator=gen) * (hi - lo) + lo).to(cuda)  # noqa: E731
    return r(0.5, 1.5), r(-0.3, 0.3), r(-0.5, 0.5), r(0.5, 1.5)


def _affine64(x, bn):
    """float64 BN(x) of bf16 rows x from the running statistics, and its fp32 evaluation bound e_v."""
    w, b, rm, rv = (t.double() for t in bn)
    x = x.double()
    eps = float(np.float32(EPS))
    inv = (rv + eps) ** -0.5
    v = (x - rm) * inv * w + b
    sc = w * inv
    sh = b - rm * sc
    e_sc = w.abs() * 2.5 * U * inv + U * sc.abs()
    e_sh = rm.abs() * e_sc + U * (rm * sc).abs() + U * sh.abs()
    return v, x.abs() * e_sc + e_sh + U * (x * sc).abs() + U * v.abs()


def _check(what, got, v, e, relu):
    lo_v, hi_v = (v - e, v + e)
    near = int((v.abs() < 2.0 ** 9 * e).sum())  # where fp32 cannot resolve the bf16 neighbours of v
    if relu:
        lo_v, hi_v, v = lo_v.clamp_min(0.0), hi_v.clamp_min(0.0), v.clamp_min(0.0)
    lo, hi = bf16_floor_ceil(lo_v)[0], bf16_floor_ceil(hi_v)[1]
    g = got.double()
    assert bool(torch.isfinite(g).all()), what
    bad = int(((g < lo) | (g > hi)).sum())
    slo, shi = bf16_floor_ceil(v)
    strict = int(((g < slo) | (g > shi)).sum())
    print(f"bn-eval | {what} | outside bound {bad}, outside the plain neighbours {strict} (elements at "
          f"cancellation {near}) of {g.numel()}")
    assert bad == 0 and strict <= near, what


SHAPES = [(37, 64, 1, 37, 1), (37, 24, 1, 1, 37), (4 * 7 * 7, 2048, 4, 7, 7)]  # M, C and the N, H, W they are run as


@pytest.mark.parametrize("M,C,N,H,W", SHAPES)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_bn_act_eval_fp64(cuda, M, C, N, H, W, relu, with_res):
    gen = torch.Generator().manual_seed(M * 31 + C)
    bn = _bn(C, gen, cuda)
    x = (torch.randn(M, C, generator=gen) * 1.5 + 0.2).to(BF16).to(cuda)
    res = torch.randn(M, C, generator=gen).to(BF16).to(cuda) if with_res else None
    keep = [t.clone() for t in (x, *bn)] + ([res.clone()] if with_res else [])
    y = _m().bn_act_eval(nhwc(x, N, H, W), nhwc(res, N, H, W) if with_res else None, bn[0], bn[1], bn[2], bn[3],
                         EPS, relu)
    assert y.dtype == BF16 and y.shape == (N, C, H, W) and y.is_contiguous(memory_format=torch.channels_last)
    v, e = _affine64(x, bn)
    if with_res:
        v = v + res.double()
        e = e + U * v.abs()
    _check(f"act M {M} C {C} relu {relu} res {with_res}", rows_of(y), v, e, relu)
    now = [x, *bn] + ([res] if with_res else [])
    assert all(torch.equal(a, b) for a, b in zip(keep, now))  # inputs and running statistics untouched


@pytest.mark.parametrize("M,C,N,H,W", SHAPES)
@pytest.mark.parametrize("relu", [False, True])
def test_bn_act_eval_pair_fp64(cuda, M, C, N, H, W, relu):
    gen = torch.Generator().manual_seed(M * 37 + C)
    bn, rbn = _bn(C, gen, cuda), _bn(C, gen, cuda)
    x = (torch.randn(M, C, generator=gen) * 1.5 + 0.2).to(BF16).to(cuda)
    r = (torch.randn(M, C, generator=gen) - 0.3).to(BF16).to(cuda)
    keep = [t.clone() for t in (x, r, *bn, *rbn)]
    y = _m().bn_act_eval_pair(nhwc(x, N, H, W), bn[0], bn[1], bn[2], bn[3], EPS, nhwc(r, N, H, W), rbn[0], rbn[1],
                              rbn[2], rbn[3], EPS, relu)
    v1, e1 = _affine64(x, bn)
    v2, e2 = _affine64(r, rbn)
    v = v1 + v2
    _check(f"pair M {M} C {C} relu {relu}", rows_of(y), v, e1 + e2 + U * v.abs(), relu)
    assert all(torch.equal(a, b) for a, b in zip(keep, (x, r, *bn, *rbn)))


def test_bn_relu_pool_eval_fp64(cuda):
    N, H, W, C = 2, 10, 10, 64
    gen = torch.Generator().manual_seed(5)
    bn = _bn(C, gen, cuda)
    x = (torch.randn(N * H * W, C, generator=gen) * 1.5).to(BF16).to(cuda)
    keep = [t.clone() for t in (x, *bn)]
    y = _m().bn_relu_pool_eval(nhwc(x, N, H, W), *bn, EPS)
    assert y.shape == (N, C, 5, 5) and y.is_contiguous(memory_format=torch.channels_last)
    v, e = _affine64(x, bn)
    # each activation rounds to bf16 before the maximum, and the maximum is monotone: pool the
    # per-element lower and upper bf16 bounds
    lo = bf16_floor_ceil((v - e).clamp_min(0.0))[0]
    hi = bf16_floor_ceil((v + e).clamp_min(0.0))[1]
    pool = lambda t: torch.nn.functional.max_pool2d(nhwc(t, N, H, W), 3, 2, 1)  # noqa: E731
    g = y.double()
    bad = int(((g < pool(lo)) | (g > pool(hi))).sum())
    slo, shi = bf16_floor_ceil(v.clamp_min(0.0))
    strict = int(((g < pool(slo)) | (g > pool(shi))).sum())
    print(f"bn-eval | pool | outside bound {bad}, outside the plain neighbours {strict} of {g.numel()}")
    assert bad == 0 and strict <= int((v.abs() < 2.0 ** 9 * e).sum())
    assert all(torch.equal(a, b) for a, b in zip(keep, (x, *bn)))


# HIP error vs fp32 ≤ ANCHOR_RATIO × the framework-bf16 error + ANCHOR_FLOOR: the bound of
# test_workloads_gpu.test_resnet50_width_hip_vs_fp32 and its justification (bf16's own error)
ANCHOR_RATIO, ANCHOR_FLOOR = 1.5, 0.005


def test_resnet50_eval_hip_vs_fp32(cuda):
    """Full-width ResNet-50 in eval mode on the production HIP path (shadow weights + autocast, every
    convolution hand-written, BatchNorm from the running statistics) against the same weights in
    fp32 on the framework ops (CPU), anchored to the framework's own bf16 eval error.  No
    framework convolution may run: the nn.Conv2d modules are never called on the HIP path."""
    from paddle_operator_amd.models.resnet import resnet50
    from paddle_operator_amd.ops import resnet as R
    from paddle_operator_amd.parallel.flat import FlatParams

    torch.manual_seed(0)
    ref = resnet50()
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.uniform_(m.bias, -0.1, 0.1)
            torch.nn.init.uniform_(m.running_mean, -0.2, 0.2)
            torch.nn.init.uniform_(m.running_var, 0.5, 1.5)
        if hasattr(m, "bn3"):
            torch.nn.init.uniform_(m.bn3.weight, 0.1, 0.3)
    ref.eval()
    hip = copy.deepcopy(ref).to(cuda).to(memory_format=torch.channels_last)
    fw = copy.deepcopy(ref).to(cuda).to(memory_format=torch.channels_last)
    flat = FlatParams(hip, dtype=torch.float32, device=cuda, bucket_bytes=25 << 20)
    flat.enable_shadow(torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(16, 3, 128, 128, generator=g)
    xh = x.to(cuda, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    stats = {k: v.clone() for k, v in hip.named_buffers()}

    calls = {"hip": 0, "fw": 0}
    hooks = []
    for name, model in (("hip", hip), ("fw", fw)):
        for mod in model.modules():
            if isinstance(mod, torch.nn.Conv2d):
                hooks.append(mod.register_forward_hook(lambda *_a, _n=name: calls.__setitem__(_n, calls[_n] + 1)))
    used0 = R._EVAL_USED[0]
    with torch.no_grad():
        with flat.shadow_scope(), torch.autocast("cuda", dtype=torch.bfloat16):
            logits_h = hip(xh)
        used = R._EVAL_USED[0] - used0
        os.environ["PDO_OPS"] = "torch"
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits_f = fw(xh)
        finally:
            os.environ["PDO_OPS"] = "hip"
        torch.cuda.synchronize()
        logits_r = ref(x)
    for h in hooks:
        h.remove()
    n_bn = sum(isinstance(m, torch.nn.BatchNorm2d) for m in ref.modules())
    assert calls == {"hip": 0, "fw": n_bn} and used == n_bn == 53, (calls, used, n_bn)
    assert not hip.training and all(torch.equal(v, stats[k]) for k, v in hip.named_buffers())

    def rel(a, b):
        a, b = a.detach().float().cpu(), b.detach().float().cpu()
        return float((a - b).norm() / (b.norm() + 1e-12))

    eh, ef = rel(logits_h, logits_r), rel(logits_f, logits_r)
    print(f"resnet50-eval | logits rel err hip {eh:.5f} framework-bf16 {ef:.5f}")
    assert eh <= ANCHOR_RATIO * ef + ANCHOR_FLOOR, (eh, ef)
