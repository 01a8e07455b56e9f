"""Float64 reference of the depthwise 3x3 convolution (pad 1, stride 1 | 2) in NHWC, for test_gpu_depthwise_forms.py (checked against
torch.nn.functional.conv2d by test_depthwise_ref.py).

Every function is nine shifted multiply-adds over a zero-padded array - no convolution routine, so it shares nothing with the
torch.nn.Conv2d reference of test_gpu_shufflenet.py.  x, dy: (N, H, W, C) / (N, P, Q, C); w: the (C, 1, 3, 3) parameter in any shape
that flattens to [C][9]; tap k = 3 r + s reads input pixel (stride p + r - 1, stride q + s - 1).
"""
import torch

F64 = torch.float64


def out_size(n, stride):
    return (n + 2 - 3) // stride + 1


def _padded(x):
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=F64)
    xp[:, 1:H + 1, 1:W + 1] = x
    return xp


def _window(a, r, s, P, Q, stride):
    """the (N, P, Q, C) view of a padded array that tap (r, s) pairs with the output map"""
    return a[:, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride]


def forward(x, w, stride):
    N, H, W, C = x.shape
    P, Q = out_size(H, stride), out_size(W, stride)
    xp, wk = _padded(x), w.to(F64).reshape(C, 9)
    y = torch.zeros(N, P, Q, C, dtype=F64)
    for r in range(3):
        for s in range(3):
            y.addcmul_(_window(xp, r, s, P, Q, stride), wk[:, 3 * r + s])
    return y


def dgrad(dy, w, H, W, stride):
    N, P, Q, C = dy.shape
    assert (P, Q) == (out_size(H, stride), out_size(W, stride))
    g, wk = dy.to(F64), w.to(F64).reshape(C, 9)
    dxp = torch.zeros(N, H + 2, W + 2, C, dtype=F64)
    for r in range(3):
        for s in range(3):
            _window(dxp, r, s, P, Q, stride).addcmul_(g, wk[:, 3 * r + s])
    return dxp[:, 1:H + 1, 1:W + 1].contiguous()


def wgrad(dy, x, stride):
    """(dw, s_abs), both [C][9]: dw[c][k] = sum over output pixels of dy * x(tap k), s_abs the same sum over |dy * x|"""
    N, H, W, C = x.shape
    P, Q = out_size(H, stride), out_size(W, stride)
    assert tuple(dy.shape) == (N, P, Q, C)
    xp, g = _padded(x), dy.to(F64)
    dw = torch.zeros(C, 9, dtype=F64)
    s_abs = torch.zeros(C, 9, dtype=F64)
    for r in range(3):
        for s in range(3):
            prod = _window(xp, r, s, P, Q, stride) * g
            dw[:, 3 * r + s] = prod.sum(dim=(0, 1, 2))
            s_abs[:, 3 * r + s] = prod.abs_().sum(dim=(0, 1, 2))
    return dw, s_abs
