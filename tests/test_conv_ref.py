"""CPU: conv_ref (the tap-loop reference of the convolution gather-form tests) against torch.nn.functional.conv2d and autograd in float64,
on geometries of the case table: stride (2, 1) through stride_w, R != S, pad > R // 2, a map narrower than the filter, stride 3.
Agreement to 1e-12 relative (two float64 summations in different orders over at most a few hundred terms)."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as T
import conv_ref as R

IDS = ["fwd-reg-3x3", "fwd-reg-stem-sw1", "fwd-reg-sw1-c64", "fwd-reg-1x7", "fwd-reg-7x1", "fwd-reg-pad2", "fwd-reg-w2", "fwd-reg-w1", "fwd-reg-h1",
       "fwd-reg-s2mixed", "fwd-reg-s3", "fwd-reg-5x5", "fwd-reg-7x7s2", "fwd-glds-1x1s2", "wgrad-glds-1x7", "dgrad-glds-s2-pad0"]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("cid", IDS)
def test_against_conv2d_and_autograd(cid):
    g = T.BY_ID[cid]["g"]
    gen = torch.Generator().manual_seed(len(cid) * 131 + g["H"] * 7 + g["W"])
    P, Q = R.out_hw(g)
    x = torch.randn(g["N"], g["H"], g["W"], g["C"], generator=gen, dtype=torch.float64)
    w = torch.randn(g["K"], g["R"], g["S"], g["C"], generator=gen, dtype=torch.float64)
    b = torch.randn(g["K"], generator=gen, dtype=torch.float64)
    dy = torch.randn(g["N"], P, Q, g["K"], generator=gen, dtype=torch.float64)
    old = torch.randn(g["N"], g["H"], g["W"], g["C"], generator=gen, dtype=torch.float64)
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_()
    wt = w.permute(0, 3, 1, 2).clone().requires_grad_()
    y = F.conv2d(xt, wt, b, stride=R.strides(g), padding=g["pad"])
    assert tuple(y.shape) == (g["N"], g["K"], P, Q)
    y.backward(dy.permute(0, 3, 1, 2))
    assert _rel(R.forward(g, x, w, b), y.detach().permute(0, 2, 3, 1)) <= 1e-12
    assert _rel(R.forward(g, x, w), (y.detach() - b[None, :, None, None]).permute(0, 2, 3, 1)) <= 1e-12
    dx, prod = R.dgrad(g, dy, w)
    assert torch.equal(dx, prod) and _rel(dx, xt.grad.permute(0, 2, 3, 1)) <= 1e-12
    dxa, prod = R.dgrad(g, dy, w, dx_old=old, accumulate=True)
    assert _rel(dxa, old + xt.grad.permute(0, 2, 3, 1)) <= 1e-12 and _rel(prod, xt.grad.permute(0, 2, 3, 1)) <= 1e-12
    assert _rel(R.wgrad(g, dy, x), wt.grad.permute(0, 2, 3, 1)) <= 1e-12


def test_rounding_option_rounds_the_inputs_only():
    g = R.geom(2, 5, 6, 8, 8, 3, 3, 2, 1)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 6, 8, generator=gen); w = torch.randn(8, 3, 3, 8, generator=gen); b = torch.randn(8, generator=gen)
    want = R.forward(g, R.bf16_round(x), R.bf16_round(w), b)
    assert torch.equal(R.forward(g, x, w, b, round_inputs_to_bf16=True), want)
    assert not torch.equal(R.forward(g, x, w, b), want)
    P, Q = R.out_hw(g)
    dy = torch.randn(2, P, Q, 8, generator=gen)
    assert torch.equal(R.dgrad(g, dy, w, round_inputs_to_bf16=True)[0], R.dgrad(g, R.bf16_round(dy), R.bf16_round(w))[0])
    assert torch.equal(R.wgrad(g, dy, x, round_inputs_to_bf16=True), R.wgrad(g, R.bf16_round(dy), R.bf16_round(x)))
