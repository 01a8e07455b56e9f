"""float64 reference of ONE step of the fused optimizer (csrc/optimizer.hip), written out as in the header comment of include/sat_hip.h,
with a running error analysis beside every value.  No import of the library.  test_optimizer_ref.py checks it against torch.optim on
float64 CPU tensors before test_gpu_optimizer_forms.py lets it judge a kernel.

Every quantity is a ``T``: the float64 value ``v``, a magnitude ``mag >= |v|`` and a count ``k`` such that the fp32 evaluation of the same
expression is, to first order in u = 2^-24, within ``k * u * mag`` of ``v``.  Inputs are exact (mag = |v|, k = 0).  One fp32 operation
rounds once (relative error u of its own result) and hands on the errors of its operands:

    z = x +- y       mag = mag x + mag y                 k = max(kx, ky) + 1
    z = x * y        mag = mag x * mag y                 k = kx + ky + 1          (|y| ex + |x| ey + u |z|)
    z = fma(x, y, w) mag = mag x * mag y + mag w         k = max(kx + ky, kw) + 1 (one rounding)
    z = x / y        mag = |z| (mag x/|x|) (mag y/|y|)   k = kx + ky + 1          (relative errors add)
    z = sqrt(x)      mag = |z| (mag x/|x|)               k = kx + 1               (the relative error halves: counted whole)
    select / clamp   exact

``mag`` is "the sum of the magnitudes of the terms" of the expression (for p of plain SGD: |p| + |lr g|), carried through products and
quotients so that a cancellation upstream (m + (g - m)(1 - beta1) near 0) widens the bound of what is computed from it.  ``k`` depends
on the expression only, never on the data: K_TABLE at the bottom lists it per kind and stream, test_optimizer_ref.py pins the table.

The expressions are those of opt_update / asgd_update / avg_elem with every C operator as one rounding, the explicit fmaf()s as one.
The file is compiled with contraction on, and the compiler does fuse some a * b + c (and not others: the 16-byte loop of
optimizer_step_kernel computes beta2 * v and ((1 - beta2) g) g with one packed multiply and adds them, and multiplies lr by the update
before it subtracts).  A contraction removes a rounding, so the uncontracted count bounds either choice.  fp32 `/` and sqrtf are the
correctly rounded sequences in the generated gfx950 code (v_div_scale / v_div_fmas / v_div_fixup; v_sqrt_f32 followed by the two
fma residual tests that step the result by one ulp): one rounding each.
"""
import math

import numpy as np

U = 2.0 ** -24
SGD, ADAM, ADAMW, ASGD = 0, 1, 2, 3


class T:
    __slots__ = ("v", "mag", "k")

    def __init__(self, v, mag=None, k=0):
        self.v = np.asarray(v, dtype=np.float64)
        self.mag = np.abs(self.v) if mag is None else np.asarray(mag, dtype=np.float64)
        self.k = int(k)

    def bound(self):
        """k u mag per element"""
        return self.k * U * self.mag


def _t(x):
    return x if isinstance(x, T) else T(x)


def add(x, y):
    x, y = _t(x), _t(y)
    with np.errstate(all='ignore'):
        return T(x.v + y.v, x.mag + y.mag, max(x.k, y.k) + 1)


def sub(x, y):
    x, y = _t(x), _t(y)
    with np.errstate(all='ignore'):
        return T(x.v - y.v, x.mag + y.mag, max(x.k, y.k) + 1)


def mul(x, y):
    x, y = _t(x), _t(y)
    with np.errstate(all='ignore'):
        return T(x.v * y.v, x.mag * y.mag, x.k + y.k + 1)


def fma(x, y, w):
    x, y, w = _t(x), _t(y), _t(w)
    with np.errstate(all='ignore'):
        return T(x.v * y.v + w.v, x.mag * y.mag + w.mag, max(x.k + y.k, w.k) + 1)


def _spread(x):
    """mag / |v| >= 1 (1 where the value is 0 and so is its magnitude)"""
    with np.errstate(all="ignore"):
        r = x.mag / np.abs(x.v)
    return np.where(np.abs(x.v) == x.mag, 1.0, r)


def div(x, y):
    x, y = _t(x), _t(y)
    with np.errstate(all="ignore"):
        z = x.v / y.v
        return T(z, np.abs(z) * _spread(x) * _spread(y), x.k + y.k + 1)


def sqrt(x):
    with np.errstate(all="ignore"):
        z = np.sqrt(x.v)
        return T(z, np.abs(z) * _spread(x), x.k + 1)


# ---------------------------------------------------------------------------------------------------------------- clipping
def norm_coef(grads, max_norm):
    """(coef, norm) of torch.nn.utils.clip_grad_norm_ in float64: norm = sqrt(sum g^2) over all tensors, coef = min(1, max_norm /
    (norm + 1e-6)); a NaN norm gives a NaN coefficient (torch.clamp keeps NaN), an infinite one gives 0"""
    s = 0.0
    with np.errstate(all="ignore"):
        for g in grads:
            g = np.asarray(g, dtype=np.float64).reshape(-1)
            s += float(np.sum(g * g))
    norm = math.sqrt(s) if s == s else float("nan")
    c = max_norm / (norm + 1e-6)
    return (c if c != c else min(1.0, c)), norm


def clipped_grad(g, coef, clip_value):
    """g * coef (coef None = no norm clipping: the kernel multiplies by 1.f, exactly), then torch.nn.utils.clip_grad_value_: clamp to
    [-c, c], NaN stays NaN, +-inf become +-c"""
    g = _t(g)
    if coef is not None:
        g = mul(g, coef)
    if clip_value > 0:
        with np.errstate(all="ignore"):
            v = np.clip(g.v, -clip_value, clip_value)          # np.minimum / np.maximum hand a NaN on
            g = T(v, np.where(np.isnan(g.mag), g.mag, np.minimum(g.mag, clip_value)), g.k)
    return g


# ---------------------------------------------------------------------------------------------------------------- the updates
def sgd(p, g, m, lr, wd, momentum=0.0, nesterov=False, first_step=False):
    """-> (p, m); m is None when momentum == 0 (the buffer is not written)"""
    p, g = _t(p), _t(g)
    if wd != 0:
        g = fma(wd, p, g)
    m_new = None
    if momentum != 0:
        m_new = g if first_step else fma(momentum, m, g)          # torch: buf = grad on the first step
        g = fma(momentum, m_new, g) if nesterov else m_new
    return sub(p, mul(lr, g)), m_new


def _adam_tail(p, g, m, v, lr, beta1, beta2, eps, bc1, bc2_sqrt):
    m, v = _t(m), _t(v)
    m_new = add(m, mul(sub(g, m), sub(1.0, beta1)))                                # exp_avg.lerp_(grad, 1 - beta1)
    v_new = add(mul(beta2, v), mul(mul(sub(1.0, beta2), g), g))
    denom = add(div(sqrt(v_new), bc2_sqrt), eps)
    return sub(p, mul(div(lr, bc1), div(m_new, denom))), m_new, v_new


def adam(p, g, m, v, lr, wd, beta1, beta2, eps, bc1, bc2_sqrt):
    """the L2 term joins the gradient -> (p, m, v)"""
    p, g = _t(p), _t(g)
    if wd != 0:
        g = fma(wd, p, g)
    return _adam_tail(p, g, m, v, lr, beta1, beta2, eps, bc1, bc2_sqrt)


def adamw(p, g, m, v, lr, wd, beta1, beta2, eps, bc1, bc2_sqrt):
    """decoupled decay: p *= 1 - lr wd first -> (p, m, v)"""
    p = mul(p, sub(1.0, mul(lr, wd)))
    return _adam_tail(p, _t(g), m, v, lr, beta1, beta2, eps, bc1, bc2_sqrt)


def asgd(p, g, eta, wd, lambd):
    """g += wd p;  p = p (1 - lambd eta) - eta g"""
    p, g = _t(p), _t(g)
    if wd != 0:
        g = fma(wd, p, g)
    p = mul(p, fma(-lambd, eta, 1.0))
    return fma(-eta, g, p)


def average(a, p, coef):
    """a = coef == 1 ? p : a + (p - a) coef"""
    if coef == 1:
        return p
    return add(a, mul(sub(p, a), coef))


def step(hyper, lr, wd, p, g, m=None, v=None, a=None, avg=None, coef=None):
    """One element-wise step.  hyper: the fields of sat_opt_hyper as a dict (kind, nesterov, first_step, beta1, beta2, eps,
    bias_correction1, bias_correction2_sqrt, momentum, clip_value); avg: None or the fields of sat_opt_avg_hyper (coef, lambd);
    coef: None or the norm-clip coefficient.  Returns {"p": T, "m": T | None, "v": T | None, "a": T | None}: None = not written."""
    kind = hyper["kind"]
    gc = clipped_grad(g, coef, hyper.get("clip_value", 0.0))
    out = dict(p=None, m=None, v=None, a=None)
    if kind == SGD:
        out["p"], out["m"] = sgd(p, gc, m, lr, wd, hyper.get("momentum", 0.0), bool(hyper.get("nesterov", 0)), bool(hyper.get("first_step", 0)))
    elif kind in (ADAM, ADAMW):
        f = adam if kind == ADAM else adamw
        out["p"], out["m"], out["v"] = f(p, gc, m, v, lr, wd, hyper["beta1"], hyper["beta2"], hyper["eps"], hyper["bias_correction1"],
                                         hyper["bias_correction2_sqrt"])
    elif kind == ASGD:
        if avg is None:
            raise ValueError("ASGD is a kind of the averaging step only")
        out["p"] = asgd(p, gc, lr, wd, avg["lambd"])
    else:
        raise ValueError("kind %r" % (kind,))
    if avg is not None and a is not None:
        out["a"] = average(_t(a), out["p"], avg["coef"])
    return out


def k_table():
    """k per (kind, stream) for the settings that lengthen the path (weight decay, norm and value clipping on, momentum with nesterov, a
    coefficient below 1): the numbers the module docstring of test_gpu_optimizer_forms.py quotes"""
    one = np.ones(1)
    h = dict(nesterov=1, first_step=0, beta1=0.9, beta2=0.999, eps=1e-8, bias_correction1=0.1, bias_correction2_sqrt=0.03, momentum=0.9, clip_value=10.0)
    table = {}
    for name, kind in (("sgd", SGD), ("adam", ADAM), ("adamw", ADAMW), ("asgd", ASGD)):
        r = step(dict(h, kind=kind), 0.01, 0.05, one, one, one, one, one, avg=dict(coef=0.5, lambd=1e-2), coef=0.5)
        table[name] = {s: t.k for s, t in r.items() if t is not None}
    return table


#: pinned by test_optimizer_ref.py
K_TABLE = {"sgd": {"p": 6, "m": 3, "a": 9}, "adam": {"p": 21, "m": 6, "v": 8, "a": 24}, "adamw": {"p": 18, "m": 5, "v": 6, "a": 21},
           "asgd": {"p": 3, "a": 6}}
