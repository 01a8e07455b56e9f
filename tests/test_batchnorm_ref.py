"""CPU: the float64 references of tests/batchnorm_ref.py against torch's own batch_norm / max_pool2d and autograd in float64, so that the
GPU comparison of test_gpu_batchnorm_forms.py stands on a reference that is itself checked."""
import pytest
import torch
import torch.nn.functional as F

import batchnorm_ref as R

F64 = torch.float64


@pytest.mark.parametrize("relu", (0, 1, 2))
def test_batchnorm_reference_matches_autograd(relu):
    torch.manual_seed(relu)
    rows, C = 37, 16
    x, res = (torch.randn(rows, C, dtype=F64, requires_grad=True) for _ in range(2))
    gamma, beta = (torch.randn(C, dtype=F64, requires_grad=True) for _ in range(2))
    dy = torch.randn(rows, C, dtype=F64)
    run_mean, run_var = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    v = F.batch_norm(x, run_mean, run_var, gamma, beta, True, 0.1, 1e-5) + 2.0 * res
    y = v if relu == 0 else (v.clamp(min=0) if relu == 1 else F.hardtanh(v, 0.0, 6.0))
    gx, gg, gb, gr = torch.autograd.grad(y, (x, gamma, beta, res), dy)
    xd = x.detach()
    mean, var, invstd, unbiased = R.train_stats(xd, 1e-5)
    yr, bits, vr = R.forward(xd, mean, invstd, gamma.detach(), beta.detach(), 2.0 * res.detach(), relu)
    b = R.backward(xd, dy, bits, mean, invstd, gamma.detach(), relu)
    for got, want in ((yr, y), (b["dx"], gx), (b["dgamma"], gg), (b["dbeta"], gb), (2.0 * b["g"], gr), (0.1 * mean, run_mean), (0.9 + 0.1 * unbiased, run_var)):
        assert float((got - want.detach()).abs().max()) < 1e-12
    assert torch.equal(R.unpack_mask(R.pack_mask(bits), bits.numel()).reshape(bits.shape), bits)
    ev = R.eval_forward(xd, mean, var, 1e-5, gamma.detach(), beta.detach(), None, 0)
    assert float((ev - F.batch_norm(xd, mean, var, gamma.detach(), beta.detach(), False, 0.0, 1e-5)).abs().max()) < 1e-12


def test_tile_statistics_match_the_pass():
    torch.manual_seed(5)
    x = torch.randn(61, 8, dtype=F64).float().to(F64)
    mean, var, invstd, unbiased = R.train_stats(x, 1e-5)
    tiles = R.tile_sums(x, 4)
    assert tiles.shape == (16, 8, 2)
    tm, tv, ti, tu = R.stats_from_tiles(tiles, 61, 1e-5)
    assert float((tm - mean).abs().max()) < 1e-6 and float((ti - invstd).abs().max()) < 1e-5 and float((tu - unbiased).abs().max()) < 1e-5
    one = R.train_stats(x[:1], 1e-5)
    assert torch.equal(one[1], torch.zeros(8, dtype=F64)) and torch.equal(one[3], one[1])          # one row: no n / (n - 1)


@pytest.mark.parametrize("shape", ((2, 11, 12, 8), (1, 7, 9, 12), (1, 1, 1, 4), (1, 2, 5, 4)))
@pytest.mark.parametrize("nans", (False, True))
def test_maxpool_reference_matches_torch(shape, nans):
    torch.manual_seed(sum(shape))
    N, H, W, C = shape
    x = (torch.randint(-2, 3, shape).to(F64)).clamp(min=0.0)          # many exact ties
    if nans:
        x = torch.where(torch.rand(shape) < 0.1, torch.full_like(x, float("nan")), x)
    y, arg = R.maxpool_fwd(x)
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    yt, idx = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    assert torch.equal(torch.nan_to_num(yt.detach().permute(0, 2, 3, 1), nan=-1.0), torch.nan_to_num(y, nan=-1.0))
    P, Q = R.pool_size(H), R.pool_size(W)
    p, q = torch.arange(P).view(1, 1, P, 1), torch.arange(Q).view(1, 1, 1, Q)
    k = ((idx // W - (2 * p - 1)) * 3 + (idx % W - (2 * q - 1))).permute(0, 2, 3, 1)
    assert torch.equal(k.to(torch.uint8), arg)
    dy = torch.randn(N, P, Q, C, dtype=F64)
    gx, = torch.autograd.grad(yt, xt, dy.permute(0, 3, 1, 2))
    dx, s_abs = R.maxpool_bwd(dy, arg, H, W)
    assert torch.equal(gx.permute(0, 2, 3, 1), dx) or float((gx.permute(0, 2, 3, 1) - dx).abs().max()) < 1e-12
    assert bool((s_abs >= dx.abs() - 1e-12).all())
