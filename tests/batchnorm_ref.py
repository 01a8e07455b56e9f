"""Float64 references of BatchNorm (training and eval mode, forward and backward, with the fused residual add, ReLU / ReLU6 and the
projection shortcut's own BatchNorm) and of the 3x3 stride-2 pad-1 max pool, written from the definitions and independent of the library
and of encoder.py.  Everything is torch float64 on the CPU over a (rows, C) or (N, H, W, C) tensor; the callers round inputs to the storage
type first, so the references work on the values the kernels read.

Conventions shared with the C ABI (include/sat_hip.h):
  relu        0 none, 1 ReLU, 2 ReLU6 (clamp to [0, 6])
  pass bits   "the gradient passes": v > 0 (ReLU), 0 < v < 6 (ReLU6) of the value v before the activation
  mask bytes  bit i of byte b <-> element 8 b + i of the row-major activation
  argmax      window position kh * 3 + kw of the first maximum in scan order; a NaN beats everything, the last NaN of a window stays
"""
import torch

F64 = torch.float64


def to_storage(t, bf):
    """round a float64 / float32 tensor to the storage type and return it as float64"""
    return (t.to(torch.bfloat16) if bf else t.to(torch.float32)).to(F64)


def ulp32(t):
    """spacing of float32 at |t| (t float64), at least the smallest normal spacing"""
    a = t.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(F64)


# ------------------------------------------------------------------ statistics
def train_stats(x, eps):
    """x (rows, C) float64 -> mean, biased variance, invstd = 1 / sqrt(var + eps), unbiased variance (the running value's; one row: the biased one)"""
    rows = x.shape[0]
    mean = x.sum(0) / rows
    var = ((x - mean) ** 2).sum(0) / rows
    unbiased = var * rows / (rows - 1) if rows > 1 else var.clone()
    return mean, var, 1.0 / torch.sqrt(var + eps), unbiased


def tile_sums(x, tile_rows):
    """per row tile and channel (sum, sum of squares) in float32: what a convolution epilogue leaves; (ntiles, C, 2) float32"""
    rows, C = x.shape
    nt = -(-rows // tile_rows)
    pad = torch.zeros(nt * tile_rows - rows, C, dtype=F64)
    xt = torch.cat([x, pad]).reshape(nt, tile_rows, C)
    return torch.stack([xt.sum(1), (xt * xt).sum(1)], dim=2).to(torch.float32)


def stats_from_tiles(tiles, rows, eps):
    """the float64 formula on the float tile values themselves: mean = S / n, var = Q / n - mean^2 (clamped at 0)"""
    s, q = tiles[:, :, 0].to(F64).sum(0), tiles[:, :, 1].to(F64).sum(0)
    mean = s / rows
    var = (q / rows - mean * mean).clamp(min=0.0)
    unbiased = var * rows / (rows - 1) if rows > 1 else var.clone()
    return mean, var, 1.0 / torch.sqrt(var + eps), unbiased


def running_update(old, new, momentum):
    """(1 - m) old + m float(new), in fp32 like nn.BatchNorm2d's buffers; old float32, new float64 -> float64"""
    m = torch.tensor(momentum, dtype=torch.float32)
    return ((1 - m) * old + m * new.to(torch.float32)).to(F64)


# ------------------------------------------------------------------ forward
def activate(v, relu):
    """v before the activation -> (output, pass bits)"""
    if relu == 2:
        return v.clamp(0.0, 6.0), (v > 0) & (v < 6)
    if relu == 1:
        return v.clamp(min=0.0), v > 0
    return v, v > 0


def normalize(x, mean, invstd, gamma, beta):
    return (x - mean) * invstd * gamma + beta


def forward(x, mean, invstd, gamma, beta, residual, relu):
    """y = act((x - mean) invstd gamma + beta (+ residual)): (y, pass bits, v)"""
    v = normalize(x, mean, invstd, gamma, beta)
    if residual is not None:
        v = v + residual
    y, bits = activate(v, relu)
    return y, bits, v


def shortcut_value(raw, rmean, rinvstd, rgamma, rbeta, bf):
    """the projection shortcut's normalised value, rounded to the storage type before the add (as if it had been written out)"""
    return to_storage(normalize(raw, rmean, rinvstd, rgamma, rbeta), bf)


def eval_forward(x, running_mean, running_var, eps, gamma, beta, residual, relu):
    return forward(x, running_mean, 1.0 / torch.sqrt(running_var + eps), gamma, beta, residual, relu)[0]


def pack_mask(bits):
    """(rows, C) bool -> rows * C / 8 bytes, bit i of byte b = element 8 b + i"""
    b = bits.reshape(-1, 8).to(torch.int32)
    w = (2 ** torch.arange(8, dtype=torch.int32))
    return (b * w).sum(1).to(torch.uint8)


def unpack_mask(mask, n):
    w = (2 ** torch.arange(8, dtype=torch.int32))
    return ((mask.to(torch.int32).reshape(-1, 1) & w) != 0).reshape(-1)[:n]


# ------------------------------------------------------------------ backward
def backward(x, dy, bits, mean, invstd, gamma, relu, tiles=None):
    """g = dy where the gradient passes (relu) else 0;  dbeta = sum g, dgamma = sum g xhat, dx = gamma invstd (g - dbeta / M - xhat dgamma / M).
    mean, invstd: the values the call is given (float64 copies of the floats).  tiles (ntiles, C, 2) float32: dbeta / dgamma are the float64
    sums of those tile values instead (what the tile reducers compute) and dx uses them.
    Returns dict(g, dbeta, dgamma, dx, s_abs = sum |g xhat|)."""
    M = x.shape[0]
    g = torch.where(bits, dy, torch.zeros_like(dy)) if relu else dy
    xhat = (x - mean) * invstd
    if tiles is None:
        dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    else:
        dbeta, dgamma = tiles[:, :, 0].to(F64).sum(0), tiles[:, :, 1].to(F64).sum(0)
    dx = gamma * invstd * (g - dbeta / M - xhat * dgamma / M)
    return dict(g=g, dbeta=dbeta, dgamma=dgamma, dx=dx, s_abs=(g * xhat).abs().sum(0), xhat=xhat)


def backward_tiles(g, xhat, tile_rows):
    """(sum g, sum g xhat) per row tile in float32, (ntiles, C, 2): what the data-gradient epilogue leaves"""
    rows, C = g.shape
    nt = -(-rows // tile_rows)
    pad = torch.zeros(nt * tile_rows - rows, C, dtype=F64)
    gt = torch.cat([g, pad]).reshape(nt, tile_rows, C)
    ht = torch.cat([g * xhat, pad]).reshape(nt, tile_rows, C)
    return torch.stack([gt.sum(1), ht.sum(1)], dim=2).to(torch.float32)


def dres(g, old, bf):
    """the residual's gradient: g itself, or one fp32 add to what is there and one rounding to the storage type; exact on the CPU"""
    if old is None:
        return to_storage(g, bf)
    return to_storage((g.to(torch.float32) + old.to(torch.float32)), bf)


# ------------------------------------------------------------------ max pool 3x3, stride 2, pad 1
def pool_size(n):
    return (n + 2 - 3) // 2 + 1


def maxpool_fwd(x):
    """x (N, H, W, C) float64 -> y (N, P, Q, C), argmax (N, P, Q, C) uint8"""
    N, H, W, C = x.shape
    P, Q = pool_size(H), pool_size(W)
    best = torch.full((N, P, Q, C), float("-inf"), dtype=F64)
    arg = torch.zeros((N, P, Q, C), dtype=torch.uint8)
    padded = torch.full((N, 2 * P + 1, 2 * Q + 1, C), float("-inf"), dtype=F64)          # row / column 0 = the pad; beyond H, W too
    padded[:, 1:H + 1, 1:W + 1] = x
    inside = torch.zeros((2 * P + 1, 2 * Q + 1), dtype=torch.bool)
    inside[1:H + 1, 1:W + 1] = True
    for kh in range(3):
        for kw in range(3):
            v = padded[:, kh:kh + 2 * P:2, kw:kw + 2 * Q:2]
            ok = inside[kh:kh + 2 * P:2, kw:kw + 2 * Q:2].reshape(1, P, Q, 1)
            take = ((v > best) | torch.isnan(v)) & ok          # strict >: the first maximum stays
            best = torch.where(take, v, best)
            arg = torch.where(take, torch.full_like(arg, kh * 3 + kw), arg)
    return best, arg


def maxpool_bwd(dy, arg, H, W):
    """every input position sums the outputs whose argmax points at it: (dx, sum |terms|), both (N, H, W, C) float64"""
    N, P, Q, C = dy.shape
    dx = torch.zeros((N, 2 * P + 1, 2 * Q + 1, C), dtype=F64)
    sa = torch.zeros_like(dx)
    for kh in range(3):
        for kw in range(3):
            hit = arg == kh * 3 + kw
            dx[:, kh:kh + 2 * P:2, kw:kw + 2 * Q:2] += torch.where(hit, dy, torch.zeros_like(dy))
            sa[:, kh:kh + 2 * P:2, kw:kw + 2 * Q:2] += torch.where(hit, dy.abs(), torch.zeros_like(dy))
    return dx[:, 1:H + 1, 1:W + 1].contiguous(), sa[:, 1:H + 1, 1:W + 1].contiguous()
