"""CPU yardstick of temperature-scaling calibration: the optimisation of the reference's temperature_scaling.py (lines 51-59)
restated with stock torch calls -- ``F.cross_entropy(logits / T, targets)``, autograd, ``torch.optim.SGD`` -- parameterised by
dtype.  Run in float64 it is the truth; run in float32 it is the reference as its author ran it.  Also: the closed forms the HIP
kernels implement (gradient, SGD recurrence) written out in plain Python for the CPU tests, and the seeded inputs."""
import torch
import torch.nn.functional as F

#: the reference script's constants (temperature_scaling.py:51-54)
REFERENCE = dict(init=1.5, lr=1e-2, momentum=0.8, nesterov=True, iters=70)


def nll(logits, targets, T, dtype=torch.float64):
    """(loss, dloss/dT) of F.cross_entropy(logits / T, targets) at the scalar T, through autograd, as Python floats"""
    t = torch.tensor([float(T)], dtype=dtype, requires_grad=True)
    loss = F.cross_entropy(logits.to(dtype) / t, targets.long())
    loss.backward()
    return float(loss.detach()), float(t.grad)


def fit(logits, targets, init=1.5, lr=1e-2, momentum=0.8, nesterov=True, iters=70, dtype=torch.float64):
    """The reference's loop.  Returns (T trace: iters + 1 values, loss trace: iters, gradient trace: iters) as float64 tensors."""
    x, y = logits.to(dtype), targets.long()
    t = (torch.ones(1, dtype=dtype) * init).detach().requires_grad_(True)
    opt = torch.optim.SGD([t], lr=lr, momentum=momentum, nesterov=nesterov)
    trace, losses, grads = [float(t.detach())], [], []
    for _ in range(iters):
        loss = F.cross_entropy(x / t, y)
        loss.backward()
        losses.append(float(loss.detach())); grads.append(float(t.grad))
        opt.step()
        opt.zero_grad()
        trace.append(float(t.detach()))
    return (torch.tensor(trace, dtype=torch.float64), torch.tensor(losses, dtype=torch.float64), torch.tensor(grads, dtype=torch.float64))


def closed_form(logits, targets, T):
    """loss = mean_i [log sum_j exp(x_ij / T) - x_iy / T];  dloss/dT = mean_i [x_iy - sum_j p_ij x_ij] / T^2, p_i = softmax(x_i / T);
    float64, no autograd"""
    x = logits.double()
    xy = x.gather(1, targets.long()[:, None])[:, 0]
    z = x / T
    loss = (torch.logsumexp(z, dim=1) - xy / T).mean()
    p = torch.softmax(z, dim=1)
    grad = ((xy - (p * x).sum(dim=1)) / (T * T)).mean()
    return float(loss), float(grad)


def sgd_recurrence(grad_fn, init, lr, momentum, nesterov, iters):
    """torch.optim.SGD on one scalar, written out (Python floats = float64): first step buf = g, afterwards
    buf = momentum * buf + g; step = g + momentum * buf when nesterov else buf; T -= lr * step"""
    T, buf, trace = float(init), None, [float(init)]
    for _ in range(iters):
        g = grad_fn(T)
        buf = g if buf is None else momentum * buf + g
        step = g + momentum * buf if nesterov else buf
        T = T - lr * step
        trace.append(T)
    return trace


def confident_logits(P, V, seed, boost=8.0, wrong=0.1, scale=1.0):
    """Logits of a model that is confidently right most of the time: scale * N(0, 1), +boost on the target for a share 1 - wrong of
    the rows and on a random other class for the rest.  fp32 logits (P, V), int64 targets (P,)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, V, generator=g) * scale
    y = torch.randint(0, V, (P,), generator=g)
    other = (y + torch.randint(1, V, (P,), generator=g)) % V if V > 1 else y
    hit = torch.where(torch.rand(P, generator=g) < wrong, other, y)
    x[torch.arange(P), hit] += boost
    return x, y


def bound(trace_hip, trace64, trace32):
    """(e_hip, limit, e_ref32): limit = 2 * e_ref32 + ulp, ulp = 2^-23 * max(trace64) -- "no worse than the same arithmetic in the same
    precision done in another order" plus one fp32 step of a value stored in fp32"""
    e_ref32 = float((trace32 - trace64).abs().max())
    e_hip = float((trace_hip.double() - trace64).abs().max())
    ulp = 2.0 ** -23 * float(trace64.abs().max())
    return e_hip, 2.0 * e_ref32 + ulp, e_ref32
