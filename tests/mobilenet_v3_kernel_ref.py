"""Float64 specifications of the three operations mobilenet_v3_small added, written from the definitions in include/sat_hip.h and
independent of the library and of encoder_mobilenet_v3.py (checked against torch autograd by test_mobilenet_v3_kernel_ref.py).
Everything is torch float64 on the CPU; the callers round inputs to the storage type first, so the references work on the values the
kernels read.  Next to each result come the sums of magnitudes its a-priori error bound needs.

Depthwise 5x5 (pad 2, stride 1 | 2), NHWC: x (N, H, W, C), dy (N, P, Q, C), w anything that flattens to [C][25]; tap k = 5 r + s pairs
output pixel (p, q) with input pixel (stride p + r - 2, stride q + s - 2).  25 shifted multiply-adds over a zero-padded array, no
convolution routine.

BatchNorm + hard-swish over (rows, C): v = (x - mean) invstd gamma + beta, y = v min(max(v + 3, 0), 6) / 6; the backward takes
g' = dy * slope(v) with slope = 0 for v <= -3, v / 3 + 0.5 for v < 3, else 1 (both kinks take the outer branch), then BatchNorm's backward.

Squeeze-and-excitation over x (N, HW, C): pool = mean_hw x, h = relu(w1 pool + b1), z2 = w2 h + b2, s = min(max(z2 + 3, 0), 6) / 6,
y = x s.  The backward works from the saved pool, h, z2, s it is handed: ds = sum_hw dy x, dz2 = ds / 6 where -3 < z2 < 3 else 0,
dz1 = w2^T dz2 where h > 0 else 0, dpool = w1^T dz1, dx = dy s + dpool / HW, and the parameter gradients summed over the images.
"""
import torch

F64 = torch.float64


def to_storage(t, bf):
    """round to the storage type and return float64"""
    return (t.to(torch.bfloat16) if bf else t.to(torch.float32)).to(F64)


# ------------------------------------------------------------------ depthwise 5x5
def dw5_out(n, stride):
    return (n + 4 - 5) // stride + 1


def _padded(x):
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 4, W + 4, C, dtype=F64)
    xp[:, 2:H + 2, 2:W + 2] = x
    return xp


def _window(a, r, s, P, Q, stride):
    """the (N, P, Q, C) view of a padded array that tap (r, s) pairs with the output map"""
    return a[:, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride]


def dw5_forward(x, w, stride):
    N, H, W, C = x.shape
    P, Q = dw5_out(H, stride), dw5_out(W, stride)
    xp, wk = _padded(x), w.to(F64).reshape(C, 25)
    y = torch.zeros(N, P, Q, C, dtype=F64)
    for r in range(5):
        for s in range(5):
            y.addcmul_(_window(xp, r, s, P, Q, stride), wk[:, 5 * r + s])
    return y


def dw5_dgrad(dy, w, H, W, stride):
    N, P, Q, C = dy.shape
    assert (P, Q) == (dw5_out(H, stride), dw5_out(W, stride))
    g, wk = dy.to(F64), w.to(F64).reshape(C, 25)
    dxp = torch.zeros(N, H + 4, W + 4, C, dtype=F64)
    for r in range(5):
        for s in range(5):
            _window(dxp, r, s, P, Q, stride).addcmul_(g, wk[:, 5 * r + s])
    return dxp[:, 2:H + 2, 2:W + 2].contiguous()


def dw5_wgrad(dy, x, stride):
    """(dw, s_abs), both [C][25]: dw[c][k] = sum over output pixels of dy * x(tap k), s_abs the same sum over |dy * x|"""
    N, H, W, C = x.shape
    P, Q = dw5_out(H, stride), dw5_out(W, stride)
    assert tuple(dy.shape) == (N, P, Q, C)
    xp, g = _padded(x), dy.to(F64)
    dw = torch.zeros(C, 25, dtype=F64)
    s_abs = torch.zeros(C, 25, dtype=F64)
    for r in range(5):
        for s in range(5):
            prod = _window(xp, r, s, P, Q, stride) * g
            dw[:, 5 * r + s] = prod.sum(dim=(0, 1, 2))
            s_abs[:, 5 * r + s] = prod.abs_().sum(dim=(0, 1, 2))
    return dw, s_abs


# ------------------------------------------------------------------ BatchNorm + hard-swish
def hardswish(v):
    return v * (v + 3.0).clamp(0.0, 6.0) / 6.0


def hardswish_slope(v):
    """torch's hardswish_backward: v <= -3 -> 0, v < 3 -> v / 3 + 0.5, else 1"""
    return torch.where(v <= -3.0, torch.zeros_like(v), torch.where(v < 3.0, v / 3.0 + 0.5, torch.ones_like(v)))


def bn_train_stats(x, eps):
    """x (rows, C) -> mean, biased variance, invstd = 1 / sqrt(var + eps), the unbiased variance of the running value (one row: the biased one)"""
    rows = x.shape[0]
    mean = x.sum(0) / rows
    var = ((x - mean) ** 2).sum(0) / rows
    unbiased = var * rows / (rows - 1) if rows > 1 else var.clone()
    return mean, var, 1.0 / torch.sqrt(var + eps), unbiased


def running_update(old, new, momentum):
    """(1 - m) old + m float(new) in fp32 like nn.BatchNorm2d's buffers; old float32, new float64 -> float64"""
    m = torch.tensor(momentum, dtype=torch.float32)
    return ((1 - m) * old + m * new.to(torch.float32)).to(F64)


def bn_hs_forward(x, mean, invstd, gamma, beta):
    """dict(y, v, t = (x - mean) invstd gamma: the magnitude next to beta that enters v)"""
    t = (x - mean) * invstd * gamma
    v = t + beta
    return dict(y=hardswish(v), v=v, t=t)


def bn_hs_eval_forward(x, running_mean, running_var, eps, gamma, beta):
    return bn_hs_forward(x, running_mean, 1.0 / torch.sqrt(running_var + eps), gamma, beta)


def bn_hs_backward(x, dy, mean, invstd, gamma, beta):
    """mean, invstd: the values the call is given (float64 copies of the floats).
    dict(v, t, slope, g = dy slope, xhat, dbeta = sum g, dgamma = sum g xhat, dx = gamma invstd (g - dbeta / M - xhat dgamma / M))"""
    M = x.shape[0]
    xhat = (x - mean) * invstd
    t = xhat * gamma
    v = t + beta
    slope = hardswish_slope(v)
    g = dy * slope
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    dx = gamma * invstd * (g - dbeta / M - xhat * dgamma / M)
    return dict(v=v, t=t, slope=slope, g=g, xhat=xhat, dbeta=dbeta, dgamma=dgamma, dx=dx)


# ------------------------------------------------------------------ squeeze-and-excitation
def se_forward(x, w1, b1, w2, b2):
    """x (N, HW, C), w1 (S, C), b1 (S), w2 (C, S), b2 (C) -> dict(pool, h, z2, s, y, and a_pool = mean_hw |x|, a_h = sum_c |w1 pool| + |b1|,
    a_z2 = sum_j |w2 h| + |b2|: the magnitudes that enter pool, the pre-activation of h, and z2)"""
    pool = x.mean(1)
    z1 = pool @ w1.t() + b1
    h = z1.clamp(min=0.0)
    z2 = h @ w2.t() + b2
    s = (z2 + 3.0).clamp(0.0, 6.0) / 6.0
    return dict(pool=pool, h=h, z2=z2, s=s, y=x * s[:, None, :], a_pool=x.abs().mean(1), a_h=pool.abs() @ w1.abs().t() + b1.abs(),
                a_z2=h.abs() @ w2.abs().t() + b2.abs())


def se_backward(dy, x, w1, w2, pool, h, z2, s):
    """pool, h, z2, s: the saved vectors the call is handed ([N][C] / [N][S], float64 copies of the floats).
    dict(ds, dz2, dz1, dpool, dx, dw1 (S, C), db1, dw2 (C, S), db2, and a_ds = sum_hw |dy x|, a_dz1 = sum_c |w2 dz2|, a_dpool = sum_j |w1 dz1|)"""
    HW = x.shape[1]
    ds = (dy * x).sum(1)
    dz2 = torch.where((z2 > -3.0) & (z2 < 3.0), ds / 6.0, torch.zeros_like(ds))
    live = h > 0.0
    dz1 = torch.where(live, dz2 @ w2, torch.zeros_like(h))
    dpool = dz1 @ w1
    dx = dy * s[:, None, :] + dpool[:, None, :] / HW
    return dict(ds=ds, dz2=dz2, dz1=dz1, dpool=dpool, dx=dx, dw1=dz1.t() @ pool, db1=dz1.sum(0), dw2=dz2.t() @ h, db2=dz2.sum(0),
                a_ds=(dy * x).abs().sum(1), a_dz1=torch.where(live, dz2.abs() @ w2.abs(), torch.zeros_like(h)), a_dpool=dz1.abs() @ w1.abs())
