"""CPU: the shifted-multiply-add reference of the depthwise 3x3 convolution (tests/depthwise_ref.py) against torch's grouped convolution
in double, forward and both gradients."""
import pytest
import torch
import torch.nn.functional as F

import depthwise_ref as R


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("N,H,W,C", [(2, 5, 6, 4), (1, 1, 1, 8), (3, 4, 7, 12)])
def test_reference_matches_grouped_conv2d(N, H, W, C, stride):
    g = torch.Generator().manual_seed(100 * H + 10 * W + stride)
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(C, 1, 3, 3, generator=g, dtype=torch.float64)
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_()
    wt = w.clone().requires_grad_()
    y = F.conv2d(xt, wt, None, stride, 1, groups=C)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    dy_nhwc = dy.permute(0, 2, 3, 1).contiguous()
    assert tuple(y.shape[2:]) == (R.out_size(H, stride), R.out_size(W, stride))
    tol = dict(rtol=0.0, atol=1e-12)
    torch.testing.assert_close(R.forward(x, w, stride), y.detach().permute(0, 2, 3, 1), **tol)
    torch.testing.assert_close(R.dgrad(dy_nhwc, w, H, W, stride), xt.grad.permute(0, 2, 3, 1), **tol)
    dw, s_abs = R.wgrad(dy_nhwc, x, stride)
    torch.testing.assert_close(dw, wt.grad.reshape(C, 9), **tol)
    assert bool((s_abs >= dw.abs() - 1e-12).all())
    # s_abs is the same sum over absolute values: with non-negative operands it is dw itself
    dw_pos, s_pos = R.wgrad(dy_nhwc.abs(), x.abs(), stride)
    torch.testing.assert_close(dw_pos, s_pos, **tol)
