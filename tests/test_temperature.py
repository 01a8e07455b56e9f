"""CPU: temperature-scaling calibration without a GPU -- the closed-form gradient and the SGD recurrence the HIP kernels implement
against autograd / torch.optim.SGD on the restatement (tests/temperature_ref.py), the three C entry points and their argument
validation, and the loud failure on CPU tensors."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

import temperature_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libsat_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("T", [0.25, 0.7, 1.0, 1.5, 4.0])
def test_closed_form_gradient_equals_autograd(T):
    x, y = R.confident_logits(256, 97, seed=11)
    loss_a, grad_a = R.nll(x, y, T, torch.float64)
    loss_c, grad_c = R.closed_form(x, y, T)
    assert abs(loss_a - loss_c) <= 1e-12 * max(1.0, abs(loss_a))
    assert abs(grad_a - grad_c) <= 1e-12 * max(1.0, abs(grad_a))


def test_row_maximum_does_not_depend_on_temperature():
    """max_j(x_ij / T) = max_j(x_ij) / T for T > 0: the shifted form with the maximum of the raw logits is the same function, and it is
    the only one that stays finite for a large common offset"""
    x, y = R.confident_logits(64, 97, seed=12, scale=3.0)
    x = x + 1e4
    for T in (0.25, 1.5):
        xd = x.double()
        m = xd.max(dim=1, keepdim=True).values
        d = xd - m
        e = torch.exp(d / T)
        s, w = e.sum(dim=1), (d * e).sum(dim=1)
        xt = xd.gather(1, y[:, None])[:, 0] - m[:, 0]
        loss = (torch.log(s) - xt / T).mean()
        grad = ((xt - w / s) / (T * T)).mean()
        loss_a, grad_a = R.nll(x, y, T, torch.float64)
        assert abs(float(loss) - loss_a) <= 1e-11 * max(1.0, abs(loss_a))
        assert abs(float(grad) - grad_a) <= 1e-11 * max(1.0, abs(grad_a))
        assert not math.isfinite(float(torch.exp(xd / T).sum()))          # the unshifted sum overflows even in float64


@pytest.mark.parametrize("momentum,nesterov", [(0.8, True), (0.8, False), (0.0, False)])
def test_sgd_recurrence_equals_torch_optim(momentum, nesterov):
    """The written-out recurrence has three roundings a step (momentum * buf + g, g + momentum * buf, T - lr * step); torch's
    ``add(alpha=)`` may fuse a product into its sum on some builds, which moves each by at most one unit in the last place of T.
    The fit contracts towards its optimum, so these do not grow: bound = 3 * iters * 2^-52 * max(T).  (Measured with the installed
    torch: 0 without nesterov, one unit in the last place at one step with it.)"""
    x, y = R.confident_logits(512, 200, seed=13)
    trace, _, _ = R.fit(x, y, init=1.5, lr=1e-2, momentum=momentum, nesterov=nesterov, iters=25, dtype=torch.float64)
    mine = R.sgd_recurrence(lambda T: R.nll(x, y, T, torch.float64)[1], 1.5, 1e-2, momentum, nesterov, 25)
    err = max(abs(a - b) for a, b in zip(mine, trace.tolist()))
    print("max|recurrence - torch.optim.SGD| = %.3e" % err)
    assert err <= 3 * 25 * 2.0 ** -52 * max(mine)
    assert max(mine) - min(mine) >= 0.05


def test_fit_case_of_the_issue_moves_the_temperature():
    """P = 2048, V = 1000, +8 on the target for 90 % of the rows: T goes from 1.5 down and back up, and the float32 run of the same
    loop stays within 1e-6 of the float64 one"""
    x, y = R.confident_logits(2048, 1000, seed=1)
    t64, l64, _ = R.fit(x, y, dtype=torch.float64, **R.REFERENCE)
    t32, _, _ = R.fit(x, y, dtype=torch.float32, **R.REFERENCE)
    assert float(t64.max() - t64.min()) >= 0.05 and float(t64.min()) < 1.0
    assert float((t32 - t64).abs().max()) < 1e-6
    assert l64[-1] < l64[0]


def test_symbols_exported_and_bound(lib):
    from sat_amd import _lib
    for name in ("sat_temperature_workspace_bytes", "sat_temperature_nll", "sat_temperature_fit"):
        assert name in _lib.SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1]


def test_workspace_bytes(lib):
    assert lib.sat_temperature_workspace_bytes(0, 100) == 0 and b"non-positive" in lib.sat_last_error()
    assert lib.sat_temperature_workspace_bytes(100, 0) == 0
    assert lib.sat_temperature_workspace_bytes(-3, 100) == 0
    small, big = lib.sat_temperature_workspace_bytes(1000, 6400), lib.sat_temperature_workspace_bytes(70560, 6400)
    assert 0 < small < big
    assert big == lib.sat_temperature_workspace_bytes(70560, 10000)          # no term of the size of a row
    assert big < 70560 * 64


def test_argument_validation_without_gpu(lib):
    """SAT_EINVAL (1) with a message, before anything touches the GPU: the pointers are never dereferenced"""
    p = 4096                      # any non-null value
    ok_nll = [p, p, 8, 97, p, 1, p, p, p, None]
    assert lib.sat_temperature_nll(*ok_nll[:0], None, *ok_nll[1:]) == 1 and b"null" in lib.sat_last_error()
    for i in (1, 4, 6, 7, 8):
        a = list(ok_nll); a[i] = None
        assert lib.sat_temperature_nll(*a) == 1 and b"null" in lib.sat_last_error()
    for i, bad in ((2, 0), (2, -1), (3, 0)):
        a = list(ok_nll); a[i] = bad
        assert lib.sat_temperature_nll(*a) == 1 and b"empty" in lib.sat_last_error()
    for n in (0, -1, 9):
        a = list(ok_nll); a[5] = n
        assert lib.sat_temperature_nll(*a) == 1 and b"temperatures" in lib.sat_last_error()

    ok_fit = [p, p, 8, 97, 1.5, 1e-2, 0.8, 1, 70, p, p, p, None]
    for i in (0, 1, 9, 10, 11):
        a = list(ok_fit); a[i] = None
        assert lib.sat_temperature_fit(*a) == 1 and b"null" in lib.sat_last_error()
    for i, bad in ((2, 0), (3, 0), (3, -5), (8, 0), (8, -1)):
        a = list(ok_fit); a[i] = bad
        assert lib.sat_temperature_fit(*a) == 1 and b"non-positive" in lib.sat_last_error()
    for i, bad, word in ((4, 0.0, b"initial"), (4, -1.0, b"initial"), (4, float("nan"), b"initial"), (5, 0.0, b"learning rate"),
                         (5, -1e-2, b"learning rate"), (6, -0.1, b"momentum")):
        a = list(ok_fit); a[i] = bad
        assert lib.sat_temperature_fit(*a) == 1 and word in lib.sat_last_error()


def test_python_surface_fails_loudly_on_cpu(lib):
    from sat_amd import _lib, calibration
    x, y = R.confident_logits(16, 97, seed=2)
    with pytest.raises(_lib.SatHipError):
        calibration.nll_at(x, y, [1.0])
    with pytest.raises(_lib.SatHipError):
        calibration.fit_temperature(x, y)
    from sat_amd.model import SAT
    assert callable(SAT.calibrate_temperature)
