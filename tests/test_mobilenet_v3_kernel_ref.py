"""CPU: the float64 specifications of tests/mobilenet_v3_kernel_ref.py against torch autograd in float64 (nn.Conv2d(groups = C),
BatchNorm2d + F.hardswish, mobilenet_v3_ref.SqueezeExcitationRef), and the properties of the data sets of
tests/mobilenet_v3_kernel_cases.py that test_gpu_mobilenet_v3_forms.py relies on: the "exact v" set is exact in fp32 and bf16 and puts
enough elements on and between the kinks, the "real" set puts at most 0.1 % of a case within the fp32 error of a kink, the saved SE
vectors hold their exact +-3 and zeros."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import mobilenet_v3_kernel_cases as K
import mobilenet_v3_kernel_ref as R
from mobilenet_v3_ref import SqueezeExcitationRef

F64 = torch.float64


def _close(a, b, what, tol=1e-11):
    scale = max(1.0, float(b.detach().abs().max()))
    assert float((a - b.detach()).abs().max()) <= tol * scale, what


# ------------------------------------------------------------------ depthwise 5x5
@pytest.mark.parametrize("shape", [(1, 1, 1, 4, 1), (1, 2, 3, 12, 1), (2, 7, 5, 8, 2), (2, 10, 12, 4, 2), (2, 9, 11, 8, 1)], ids=lambda s: "x".join(map(str, s)))
def test_dw5_reference_is_conv2d_with_groups(shape):
    N, H, W, C, stride = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, H, W, C, dtype=F64, generator=g)
    conv = nn.Conv2d(C, C, 5, stride, 2, groups=C, bias=False).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(C, 1, 5, 5, dtype=F64, generator=g))
    xin = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = conv(xin)
    P, Q = R.dw5_out(H, stride), R.dw5_out(W, stride)
    assert tuple(y.shape) == (N, C, P, Q)
    dy = torch.randn(N, P, Q, C, dtype=F64, generator=g)
    y.backward(dy.permute(0, 3, 1, 2))
    w = conv.weight.detach()
    _close(R.dw5_forward(x, w, stride), y.detach().permute(0, 2, 3, 1), "forward")
    _close(R.dw5_dgrad(dy, w, H, W, stride), xin.grad.permute(0, 2, 3, 1), "data gradient")
    dw, s_abs = R.dw5_wgrad(dy, x, stride)
    _close(dw, conv.weight.grad.reshape(C, 25), "filter gradient")
    assert bool((s_abs >= dw.abs() - 1e-12).all())
    # S_abs by hand for the centre tap: the output pixel (p, q) meets the input pixel (stride p, stride q)
    centre = (dy * x[:, ::stride, ::stride][:, :P, :Q]).abs().sum(dim=(0, 1, 2))
    _close(s_abs[:, 12], centre, "S_abs of the centre tap")


# ------------------------------------------------------------------ BatchNorm + hard-swish
@pytest.mark.parametrize("rows,C", [(5, 4), (37, 8), (1, 8), (300, 12)])
def test_bn_hswish_reference_is_batchnorm2d_and_hardswish(rows, C):
    g = torch.Generator().manual_seed(rows + C)
    x = 1.5 * torch.randn(rows, C, dtype=F64, generator=g) + torch.randn(C, dtype=F64, generator=g)
    dy = torch.randn(rows, C, dtype=F64, generator=g)
    bn = nn.BatchNorm2d(C, eps=K.HS_EPS, momentum=K.HS_MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(2.0 * torch.randn(C, dtype=F64, generator=g)); bn.bias.copy_(2.0 * torch.randn(C, dtype=F64, generator=g))
        bn.running_mean.copy_(torch.randn(C, dtype=F64, generator=g)); bn.running_var.copy_(0.5 + torch.rand(C, dtype=F64, generator=g))
    old_mean, old_var = bn.running_mean.clone(), bn.running_var.clone()
    gamma, beta = bn.weight.detach().clone(), bn.bias.detach().clone()

    # eval mode
    bn.eval()
    xin = x.t().reshape(1, C, rows, 1)
    _close(R.bn_hs_eval_forward(x, old_mean, old_var, K.HS_EPS, gamma, beta)["y"], F.hardswish(bn(xin)).reshape(C, rows).t(), "eval forward")

    if rows == 1:          # (torch refuses to train on one value per channel; the statistics formulas are checked on the other shapes)
        mean, var, invstd, unb = R.bn_train_stats(x, K.HS_EPS)
        assert torch.equal(mean, x[0]) and float(var.abs().max()) == 0.0 and torch.equal(unb, var)
        return
    bn.train()
    xin = xin.clone().requires_grad_(True)
    y = F.hardswish(bn(xin))
    y.backward(dy.t().reshape(1, C, rows, 1))
    mean, var, invstd, unb = R.bn_train_stats(x, K.HS_EPS)
    _close(R.bn_hs_forward(x, mean, invstd, gamma, beta)["y"], y.detach().reshape(C, rows).t(), "train forward")
    _close((1 - K.HS_MOMENTUM) * old_mean + K.HS_MOMENTUM * mean, bn.running_mean, "running mean")
    _close((1 - K.HS_MOMENTUM) * old_var + K.HS_MOMENTUM * unb, bn.running_var, "running variance (unbiased)")
    b = R.bn_hs_backward(x, dy, mean, invstd, gamma, beta)
    _close(b["dx"], xin.grad.reshape(C, rows).t(), "dx", 1e-10)
    _close(b["dgamma"], bn.weight.grad, "dgamma", 1e-10)
    _close(b["dbeta"], bn.bias.grad, "dbeta", 1e-10)
    # running_update: the fp32 update of the buffers
    got = R.running_update(old_mean.float(), mean, K.HS_MOMENTUM)
    _close(got, (1 - K.HS_MOMENTUM) * old_mean + K.HS_MOMENTUM * mean, "running_update", 1e-6)


def test_hardswish_kinks_follow_torch():
    v = torch.tensor([-4.0, -3.0, -2.999, 0.0, 2.999, 3.0, 4.0], dtype=F64, requires_grad=True)
    F.hardswish(v).sum().backward()
    assert torch.equal(R.hardswish_slope(v.detach()), v.grad)
    assert R.hardswish_slope(torch.tensor([-3.0, 3.0], dtype=F64)).tolist() == [0.0, 1.0]
    _close(R.hardswish(v.detach()), F.hardswish(v.detach()), "hardswish")


# ------------------------------------------------------------------ squeeze-and-excitation
@pytest.mark.parametrize("N,HW,C", [(1, 1, 8), (3, 6, 24), (2, 15, 72)])
def test_se_reference_is_the_torchvision_module(N, HW, C):
    g = torch.Generator().manual_seed(N * 100 + C)
    se = SqueezeExcitationRef(C).double()
    S = se.fc1.out_channels
    with torch.no_grad():
        for p, scale in ((se.fc1.weight, 2.0 / C ** 0.5), (se.fc1.bias, 0.2), (se.fc2.weight, 3.0 / S ** 0.5), (se.fc2.bias, 4.0)):
            p.copy_(scale * (2.0 * torch.rand(p.shape, dtype=F64, generator=g) - 1.0))
    x = torch.randn(N, HW, C, dtype=F64, generator=g) + torch.randn(C, dtype=F64, generator=g)
    dy = torch.randn(N, HW, C, dtype=F64, generator=g)
    w1, b1 = se.fc1.weight.detach().reshape(S, C), se.fc1.bias.detach()
    w2, b2 = se.fc2.weight.detach().reshape(C, S), se.fc2.bias.detach()
    xin = x.permute(0, 2, 1).reshape(N, C, HW, 1).clone().requires_grad_(True)
    y = se(xin)
    y.backward(dy.permute(0, 2, 1).reshape(N, C, HW, 1))
    f = R.se_forward(x, w1, b1, w2, b2)
    _close(f["y"], y.detach().reshape(N, C, HW).permute(0, 2, 1), "y")
    _close(f["s"], se.scale(xin).detach().reshape(N, C), "s")
    assert float(f["s"].min()) == 0.0 or float(f["s"].max()) == 1.0 or C == 8          # the data reaches a clamped region
    b = R.se_backward(dy, x, w1, w2, f["pool"], f["h"], f["z2"], f["s"])
    # torch's hardsigmoid_backward multiplies by the FLOAT constant 1.0f / 6.0f in every dtype (relative error 2^-26 .. 2^-25); the reference divides by 6
    SIXTH = 1e-7
    _close(b["dx"], xin.grad.reshape(N, C, HW).permute(0, 2, 1), "dx (both paths: dy s and the gradient through the scale)", SIXTH)
    _close(b["dw1"], se.fc1.weight.grad.reshape(S, C), "dw1", SIXTH)
    _close(b["db1"], se.fc1.bias.grad, "db1", SIXTH)
    _close(b["dw2"], se.fc2.weight.grad.reshape(C, S), "dw2", SIXTH)
    _close(b["db2"], se.fc2.bias.grad, "db2", SIXTH)
    # the magnitudes bound their sums
    assert bool((f["a_h"] >= f["h"] - 1e-12).all()) and bool((f["a_z2"] >= f["z2"].abs() - 1e-12).all()) and bool((f["a_pool"] >= f["pool"].abs() - 1e-12).all())
    assert bool((b["a_ds"] >= b["ds"].abs() - 1e-12).all()) and bool((b["a_dz1"] >= b["dz1"].abs() - 1e-12).all()) and bool((b["a_dpool"] >= b["dpool"].abs() - 1e-12).all())


def test_se_backward_decisions_at_the_saved_values():
    """-3 < z2 < 3 and h > 0 are read from the saved vectors: exactly +-3 and exactly 0 give exactly 0"""
    c = dict(shape=(2, 5, 8, 4))
    d = K.se_data(c, False)
    f = R.se_forward(d["x"], d["w1"], d["b1"], d["w2"], d["b2"])
    sv = K.se_saved(d, f)
    assert bool((sv["z2"][:, 0] == 3.0).all()) and bool((sv["z2"][:, -1] == -3.0).all()) and bool((sv["h"][:, 0] == 0.0).all())
    b = R.se_backward(d["dy"], d["x"], d["w1"], d["w2"], **sv)
    assert bool((b["dz2"][:, 0] == 0).all()) and bool((b["dz2"][:, -1] == 0).all()) and bool((b["dz1"][:, 0] == 0).all())
    assert bool((b["ds"][:, 0] != 0).all()) and bool((b["dz2"][:, 1:-1] != 0).any())


# ------------------------------------------------------------------ the data sets of the GPU test
def _hs_params():
    return [pytest.param(c, dtype, id="%s-%s" % (c["name"], dtype)) for c in K.HS_CASES for dtype in c["run"]]


@pytest.mark.parametrize("c,dtype", _hs_params())
def test_exact_v_set_is_exact_and_covers_the_kinks(c, dtype):
    bf = dtype == K.BF16
    d = K.hs_data(c, "exact", bf)
    x32, m32, i32, g32, b32 = (d[k].float() for k in ("x", "mean", "invstd", "gamma", "beta"))
    for t in ("x", "mean", "invstd", "gamma", "beta"):
        assert torch.equal(d[t].float().to(F64), d[t])
    if bf:
        assert torch.equal(d["x"].to(torch.bfloat16).to(F64), d["x"])
    # every fp32 operation is exact, in the kernels' association and with or without a fused multiply-add
    xh = (x32 - m32) * i32
    assert torch.equal(xh.to(F64), (d["x"] - d["mean"]) * d["invstd"])
    assert torch.equal((xh * g32 + b32).to(F64), d["v"]) and torch.equal(((x32 - m32) * i32 * g32).to(F64) + d["beta"], d["v"])
    # eval mode: eps = 0 and run_var = 1 / invstd^2 give invstd back exactly
    assert torch.equal(1.0 / torch.sqrt(d["run_var"]), i32) and torch.equal(d["run_mean"], m32)
    assert torch.equal(R.bn_hs_backward(d["x"], d["dy"], d["mean"], d["invstd"], d["gamma"], d["beta"])["v"], d["v"])
    v, n = d["v"], d["v"].numel()
    assert float((v == 3.0).sum()) >= 0.05 * n and float((v == -3.0).sum()) >= 0.05 * n
    for region in (v < -3.0, (v > -3.0) & (v < 3.0), v > 3.0):
        assert float(region.sum()) > 0.05 * n
    if c["rows"] >= 16:          # every vector lane (channel) meets both kinks
        assert bool((v == 3.0).any(0).all()) and bool((v == -3.0).any(0).all())


@pytest.mark.parametrize("c,dtype", _hs_params())
def test_real_set_keeps_away_from_the_kinks_and_reaches_every_region(c, dtype):
    bf = dtype == K.BF16
    d = K.hs_data(c, "real", bf)
    mean, var, invstd, unb = R.bn_train_stats(d["x"], K.HS_EPS)
    b = R.bn_hs_backward(d["x"], d["dy"], mean.float().to(F64), invstd.float().to(F64), d["gamma"], d["beta"])
    near = K.hs_near_kink(b["v"], b["t"], d["beta"])
    assert float(near.sum()) <= 0.001 * near.numel(), "%d element(s) within the fp32 error of a kink" % int(near.sum())
    if c["rows"] >= 20:
        v = b["v"]
        assert bool((v < -3.0).any()) and bool((v > 3.0).any()) and float(((v > -3.0) & (v < 3.0)).sum()) > 0.3 * v.numel()


@pytest.mark.parametrize("c", K.SE_CASES, ids=lambda c: "x".join(map(str, c["shape"])))
def test_se_data_reaches_every_region(c):
    d = K.se_data(c, False)
    f = R.se_forward(d["x"], d["w1"], d["b1"], d["w2"], d["b2"])
    N, HW, C, S = c["shape"]
    if C >= 16:
        assert bool((f["z2"] <= -3).any()) and bool((f["z2"] >= 3).any()) and bool(((f["z2"] > -3) & (f["z2"] < 3)).any())
    if S >= 8:
        assert bool((f["h"] > 0).any()) and bool((f["h"] == 0).any())
    sv = K.se_saved(d, f)
    b = R.se_backward(d["dy"], d["x"], d["w1"], d["w2"], **sv)
    assert bool((b["dz2"][:, 0] == 0).all()) and bool((b["dz2"][:, -1] == 0).all())
    assert S == 1 or bool((b["dz1"][:, 0] == 0).all())


@pytest.mark.parametrize("c", K.DW5_CASES, ids=lambda c: "x".join(map(str, c["shape"])))
def test_dw5_int_set_stays_exact_in_both_storage_types(c):
    d = K.dw5_data(c["shape"], "int", True)
    N, H, W, C, stride = c["shape"]
    y, dx = R.dw5_forward(d["x"], d["w"], stride), R.dw5_dgrad(d["dy"], d["w"], H, W, stride)
    dw, s_abs = R.dw5_wgrad(d["dy"], d["x"], stride)
    for t in (y, dx):
        assert float(t.abs().max()) <= 100 and torch.equal(t.to(torch.bfloat16).to(F64), t)
    assert float(s_abs.max()) < 2 ** 24 and torch.equal(dw.float().to(F64), dw)
