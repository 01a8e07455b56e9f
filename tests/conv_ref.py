"""Host reference of the dense convolutions for the gather-form tests (test_gpu_conv_forms.py; checked by test_conv_ref.py).

A float64 restatement of sat_conv2d_fwd / sat_conv2d_dgrad / sat_conv2d_wgrad for one sat_conv_geom over NHWC activations and KRSC
filters, written as explicit loops over the R x S filter taps: each tap is one strided slice of the zero-padded map times one C x K
slab of the filter.  Nothing here calls a convolution routine, so the check against torch.nn.functional.conv2d (test_conv_ref.py) is a
check of two independent statements of the operation.

A geometry is a dict with the fields of sat_conv_geom: N, H, W, C, K, R, S, stride, pad, stride_w (0 = the same as stride).
"""
import torch

F64 = torch.float64


def geom(N, H, W, C, K, R, S=None, stride=1, pad=0, stride_w=0):
    return dict(N=N, H=H, W=W, C=C, K=K, R=R, S=R if S is None else S, stride=stride, pad=pad, stride_w=stride_w)


def strides(g):
    """(vertical, horizontal) stride"""
    return g["stride"], (g["stride_w"] if g["stride_w"] > 0 else g["stride"])


def out_hw(g):
    sh, sw = strides(g)
    return (g["H"] + 2 * g["pad"] - g["R"]) // sh + 1, (g["W"] + 2 * g["pad"] - g["S"]) // sw + 1


def bf16_round(t):
    return t.float().to(torch.bfloat16).to(torch.float32)


def _prep(t, round_inputs_to_bf16):
    if round_inputs_to_bf16:
        t = bf16_round(t)
    return t.to(F64)


def _tap(g, r, s):
    """slices of the padded map that tap (r, s) reads for the P x Q outputs"""
    P, Q = out_hw(g)
    sh, sw = strides(g)
    return slice(r, r + (P - 1) * sh + 1, sh), slice(s, s + (Q - 1) * sw + 1, sw)


def _padded(g, x=None):
    p = g["pad"]
    xp = torch.zeros(g["N"], g["H"] + 2 * p, g["W"] + 2 * p, g["C"], dtype=F64)
    if x is not None:
        xp[:, p:p + g["H"], p:p + g["W"], :] = x
    return xp


def forward(g, x, w, bias=None, round_inputs_to_bf16=False):
    """x (N, H, W, C), w (K, R, S, C), bias (K) or None -> y (N, P, Q, K), float64.  The bias is never rounded (it is fp32 in memory)."""
    x, w = _prep(x, round_inputs_to_bf16), _prep(w, round_inputs_to_bf16)
    P, Q = out_hw(g)
    xp = _padded(g, x)
    y = torch.zeros(g["N"], P, Q, g["K"], dtype=F64)
    for r in range(g["R"]):
        for s in range(g["S"]):
            ys, xs = _tap(g, r, s)
            y += xp[:, ys, xs, :] @ w[:, r, s, :].t()
    if bias is not None:
        y += bias.to(F64)
    return y


def dgrad(g, dy, w, dx_old=None, accumulate=False, round_inputs_to_bf16=False):
    """dy (N, P, Q, K), w (K, R, S, C) -> (dx, prod): dx (N, H, W, C) = [dx_old +] prod, prod the gradient alone.  dx_old is taken as
    stored (the caller rounds it to the storage type)."""
    dy, w = _prep(dy, round_inputs_to_bf16), _prep(w, round_inputs_to_bf16)
    p = g["pad"]
    dxp = _padded(g)
    for r in range(g["R"]):
        for s in range(g["S"]):
            ys, xs = _tap(g, r, s)
            dxp[:, ys, xs, :] += dy @ w[:, r, s, :]
    prod = dxp[:, p:p + g["H"], p:p + g["W"], :].contiguous()
    if accumulate:
        return dx_old.to(F64) + prod, prod
    return prod, prod


def wgrad(g, dy, x, round_inputs_to_bf16=False):
    """dy (N, P, Q, K), x (N, H, W, C) -> dw (K, R, S, C), float64"""
    dy, x = _prep(dy, round_inputs_to_bf16), _prep(x, round_inputs_to_bf16)
    xp = _padded(g, x)
    dyt = dy.reshape(-1, g["K"]).t().contiguous()
    dw = torch.zeros(g["K"], g["R"], g["S"], g["C"], dtype=F64)
    for r in range(g["R"]):
        for s in range(g["S"]):
            ys, xs = _tap(g, r, s)
            dw[:, r, s, :] = dyt @ xp[:, ys, xs, :].reshape(-1, g["C"])
    return dw
