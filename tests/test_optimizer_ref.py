"""CPU: tests/optimizer_ref.py beside torch.optim on float64 tensors, before it judges a kernel (test_gpu_optimizer_forms.py).

Both sides are float64 and a step is a few dozen roundings of relative size 2^-53 ~ 1.1e-16, so they agree within 1e-12 * max(1, |ref|) per
element with three orders of magnitude to spare (cancellation in m + (g - m)(1 - beta1) included: the data are O(1))."""
import math

import numpy as np
import pytest
import torch

import averaging_ref as A
import optimizer_ref as R

SHAPES = [(5,), (33, 17), (7,), (64, 3), (1,), (129,), (2, 3, 4)]
STEPS = 4


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), want.detach().numpy().reshape(-1)
    err = np.abs(got - want)
    bound = 1e-12 * np.maximum(1.0, np.abs(want))
    assert (err <= bound).all(), (what, float(err.max()))


@pytest.mark.parametrize("kind,how", [("sgd", None), ("sgd", ("norm", 1.0)), ("sgd_plain", ("value", 0.3)), ("sgd_momentum", None), ("adam", None),
                                      ("adam", ("norm", 0.5)), ("adam", ("value", 0.02)), ("adamw", ("value", 0.02)), ("adamw", ("norm", 0.5)),
                                      ("asgd", None), ("asgd", ("norm", 0.5)), ("asgd", ("value", 0.02)), ("asgd_t0", None)])
def test_reference_matches_torch_optim_in_float64(kind, how):
    from sat_amd.optim import asgd_coefficients
    gen = torch.Generator().manual_seed(7)
    ps = [torch.randn(s, generator=gen, dtype=torch.float64).requires_grad_() for s in SHAPES]
    groups = A.groups(ps)
    lambd, alpha, t0 = 1e-2, 0.75, (2 if kind == "asgd_t0" else 1e6)
    momentum, nesterov = {"sgd": (0.9, True), "sgd_momentum": (0.9, False)}.get(kind, (0.0, False))
    beta1, beta2, eps = 0.8, 0.95, 1e-8
    if kind.startswith("asgd"):
        topt = torch.optim.ASGD(groups, lr=1e-2, lambd=lambd, alpha=alpha, t0=t0, foreach=False)
    elif kind.startswith("sgd"):
        topt = torch.optim.SGD(groups, lr=1e-2, momentum=momentum, nesterov=nesterov, foreach=False)
    elif kind == "adam":
        topt = torch.optim.Adam(groups, lr=1e-2, betas=(beta1, beta2), eps=eps, foreach=False)
    else:
        topt = torch.optim.AdamW(groups, lr=1e-2, betas=(beta1, beta2), eps=eps, weight_decay=1e-2, foreach=False)
    ema = None if kind.startswith("asgd") else A.Ema(ps, 0.9)
    # the reference's own state, as numpy float64
    P = [p.detach().numpy().copy() for p in ps]
    M = [np.zeros_like(x) for x in P]
    V = [np.zeros_like(x) for x in P]
    AV = [np.zeros_like(x) if kind.startswith("asgd") else x.copy() for x in P]
    group_of = [gi for gi, g in enumerate(topt.param_groups) for _ in g["params"]]
    etas = [float(np.float32(g["lr"])) for g in topt.param_groups]
    mu = 1.0
    for step in range(1, STEPS + 1):
        grads = [torch.randn(p.shape, generator=gen, dtype=torch.float64) * (0.1 if step % 2 else 1.0) for p in ps]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        coef = None
        if how and how[0] == "norm":
            coef, norm = R.norm_coef([g.numpy() for g in grads], how[1])
            tnorm = A.clip(ps, how)
            assert abs(norm - float(tnorm)) <= 1e-12 * norm
        elif how:
            A.clip(ps, how)
        topt.step()
        if ema is not None:
            ema.update()
        for i, g in enumerate(grads):
            grp = topt.param_groups[group_of[i]]
            hyper = dict(kind={"sgd": R.SGD, "adam": R.ADAM, "adamw": R.ADAMW, "asgd": R.ASGD}[kind.split("_")[0]], nesterov=int(nesterov),
                         first_step=int(step == 1), beta1=beta1, beta2=beta2, eps=eps, bias_correction1=1.0 - beta1 ** step,
                         bias_correction2_sqrt=math.sqrt(1.0 - beta2 ** step), momentum=momentum, clip_value=how[1] if how and how[0] == "value" else 0.0)
            if kind.startswith("asgd"):
                avg, lr = dict(coef=mu, lambd=lambd), etas[group_of[i]]
            else:
                avg, lr = dict(coef=1.0 if step == 1 else 1.0 - 0.9, lambd=0.0), grp["lr"]
            out = R.step(hyper, lr, grp["weight_decay"], P[i], g.numpy(), M[i], V[i], AV[i], avg=avg, coef=coef)
            P[i], AV[i] = out["p"].v, out["a"].v
            if out["m"] is not None:
                M[i] = out["m"].v
            if out["v"] is not None:
                V[i] = out["v"].v
            for s in ("p", "m", "v", "a"):
                if out[s] is not None:
                    assert (out[s].mag >= np.abs(out[s].v)).all()
        if kind.startswith("asgd"):          # what torch stores after this step and uses in the next (float32 0-dim tensors)
            new = [asgd_coefficients(g["lr"], lambd, alpha, t0, step) for g in topt.param_groups]
            etas, mu = [e for e, _ in new], new[0][1]
            for i, p in enumerate(ps):
                assert float(topt.state[p]["eta"]) == etas[group_of[i]] and float(topt.state[p]["mu"]) == mu
        for i, p in enumerate(ps):
            st = topt.state[p]
            _close(P[i], p, (kind, how, step, i, "p"))
            if kind.startswith("asgd"):
                _close(AV[i], st["ax"], (kind, how, step, i, "ax"))
            else:
                _close(AV[i], ema.avg[i], (kind, how, step, i, "ema"))
                if kind in ("adam", "adamw"):
                    _close(M[i], st["exp_avg"], (kind, how, step, i, "exp_avg"))
                    _close(V[i], st["exp_avg_sq"], (kind, how, step, i, "exp_avg_sq"))
                elif momentum:
                    _close(M[i], st["momentum_buffer"], (kind, how, step, i, "momentum_buffer"))
    if kind == "asgd_t0":
        assert mu < 1.0          # the running mean was reached, not only the copy


def test_non_finite_gradients_follow_torch_nn_utils():
    nan, inf = float("nan"), float("inf")
    # clip by value: NaN stays NaN, +-inf clamp
    g = torch.tensor([nan, 5.0, -5.0, inf, -inf, 0.25], dtype=torch.float64, requires_grad=True)
    g.grad = g.detach().clone()
    torch.nn.utils.clip_grad_value_([g], 0.5)
    want = g.grad.numpy()
    assert np.isnan(want[0]) and want[1:].tolist() == [0.5, -0.5, 0.5, -0.5, 0.25]
    got = R.clipped_grad(g.detach().numpy(), None, 0.5)
    assert np.isnan(got.v[0]) and got.v[1:].tolist() == want[1:].tolist()
    assert got.mag[1:].tolist() == [0.5, 0.5, 0.5, 0.5, 0.25]
    # clip by norm: a NaN anywhere makes the coefficient, and so every gradient, NaN
    a = torch.ones(3, dtype=torch.float64, requires_grad=True); b = torch.ones(2, dtype=torch.float64, requires_grad=True)
    a.grad = torch.tensor([1.0, nan, 2.0], dtype=torch.float64); b.grad = torch.tensor([3.0, 4.0], dtype=torch.float64)
    coef, norm = R.norm_coef([a.grad.numpy().copy(), b.grad.numpy().copy()], 0.5)
    tnorm = torch.nn.utils.clip_grad_norm_([a, b], 0.5)
    assert math.isnan(float(tnorm)) and math.isnan(norm) and math.isnan(coef)
    assert torch.isnan(a.grad).all() and torch.isnan(b.grad).all()
    assert np.isnan(R.clipped_grad(np.array([3.0, 4.0]), coef, 0.0).v).all()
    # an infinite norm: coefficient 0, finite gradients become 0, the infinite one NaN
    a.grad = torch.tensor([1.0, inf, 2.0], dtype=torch.float64); b.grad = torch.tensor([3.0, 4.0], dtype=torch.float64)
    coef, norm = R.norm_coef([a.grad.numpy().copy(), b.grad.numpy().copy()], 0.5)
    tnorm = torch.nn.utils.clip_grad_norm_([a, b], 0.5)
    assert float(tnorm) == inf and norm == inf and coef == 0.0
    got = R.clipped_grad(np.array([1.0, inf, 2.0]), coef, 0.0).v
    assert got[0] == 0 and np.isnan(got[1]) and got[2] == 0
    assert a.grad[0] == 0 and torch.isnan(a.grad[1]) and (b.grad == 0).all()
    # all-zero gradients: norm 0, coefficient exactly 1
    assert R.norm_coef([np.zeros(5)], 0.5) == (1.0, 0.0)


def test_k_table_is_what_the_expressions_give():
    assert R.k_table() == R.K_TABLE
    # settings that shorten the path never lengthen it
    one = np.ones(1)
    r = R.step(dict(kind=R.SGD, momentum=0.0, clip_value=0.0), 0.01, 0.0, one, one)
    assert r["p"].k == 2 and r["m"] is None and (r["p"].mag == 1.01).all()          # |p| + |lr g|: p - lr * g rounds the product and the difference
    r = R.step(dict(kind=R.SGD, momentum=0.0), 0.01, 0.0, one, one, a=one, avg=dict(coef=1.0, lambd=0.0))
    assert r["a"] is r["p"]
    r = R.step(dict(kind=R.SGD, momentum=0.0), 0.01, 0.0, one, one, a=3 * one, avg=dict(coef=0.0, lambd=0.0))
    assert (r["a"].v == 3.0).all()


def test_error_model_bounds_an_fp32_evaluation():
    """the bound holds for numpy's fp32 evaluation of the same expressions (no contraction on the CPU: every operator rounds), on data
    with cancellation: the check that the counting rules are not too tight"""
    rng = np.random.default_rng(3)
    n = 200000
    f = np.float32
    p, g, m = (rng.standard_normal(n).astype(f) for _ in range(3))
    m[::3] = g[::3] * f(1.0000001)          # g - m cancels
    v = (rng.standard_normal(n).astype(f)) ** 2
    a = rng.standard_normal(n).astype(f)
    lr, wd, b1, b2, eps, bc1, bc2, coef, cv, ac = f(0.01), f(0.05), f(0.8), f(0.95), f(1e-8), f(1 - 0.8 ** 3), f(math.sqrt(1 - 0.95 ** 3)), f(0.37), f(0.4), f(0.1)
    gc = np.clip(g * coef, -cv, cv)
    gw = (wd * p.astype(np.float64) + gc).astype(f)          # fmaf
    m32 = m + (gw - m) * (f(1) - b1)
    v32 = b2 * v + (f(1) - b2) * gw * gw
    p32 = p - (lr / bc1) * (m32 / (np.sqrt(v32) / bc2 + eps))
    a32 = a + (p32 - a) * ac
    h = dict(kind=R.ADAM, beta1=float(b1), beta2=float(b2), eps=float(eps), bias_correction1=float(bc1), bias_correction2_sqrt=float(bc2), clip_value=float(cv))
    r = R.step(h, float(lr), float(wd), p, g, m, v, a, avg=dict(coef=float(ac), lambd=0.0), coef=float(coef))
    for name, got in (("p", p32), ("m", m32), ("v", v32), ("a", a32)):
        assert got.dtype == np.float32
        ratio = np.abs(got.astype(np.float64) - r[name].v) / r[name].bound()
        print("fp32 numpy evaluation, %s: worst err / bound = %.3f (k = %d)" % (name, ratio.max(), r[name].k))
        assert ratio.max() <= 1.0
