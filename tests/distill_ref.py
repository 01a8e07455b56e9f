"""The distillation loss (include/sat_hip.h, sat_distill_fwd / _bwd; DESIGN.md 5, "Distillation") restated in float64 torch, definition by
definition.  ``distill(...)`` returns the loss, its three parts, the row terms, the row scratch and the gradient."""
import math

import torch

ARITHMETIC, GEOMETRIC = "arithmetic", "geometric"


def combined_log_q(teachers, weights, combine, inv_tau):
    """``(log q (P, V), c (P, V), [logsumexp(t_i inv_tau)] per member (None for weight 0))``: members of weight 0 are skipped"""
    ls, lses = [], []
    for t, w in zip(teachers, weights):
        if float(w) == 0.0:
            lses.append(None)
            continue
        x = t.double() * inv_tau
        lses.append(torch.logsumexp(x, -1))
        ls.append((float(w), x - lses[-1].unsqueeze(-1)))
    if combine == GEOMETRIC:
        c = sum(w * l for w, l in ls)
    else:
        assert combine == ARITHMETIC
        c = torch.logsumexp(torch.stack([l + math.log(w) for w, l in ls]), 0)
    return c - torch.logsumexp(c, -1, keepdim=True), c, lses


def distill(z, teachers, weights, combine, y, inv_tau, alpha, smoothing, g=1.0):
    z = z.double()
    P, V = z.shape
    tau = 1.0 / inv_tau
    y = y.long()
    good = (y >= 0) & (y < V)
    out = dict(hard_rows=torch.zeros(P, dtype=torch.float64), soft_rows=torch.zeros(P, dtype=torch.float64), lse=torch.zeros(P, 2, dtype=torch.float64),
               tlse=torch.zeros(P, len(teachers), dtype=torch.float64), cnorm=torch.zeros(P, dtype=torch.float64))
    grad = torch.zeros(P, V, dtype=torch.float64)
    if alpha != 1.0:                                                              # the hard term: sat_ce_label_smooth_fwd's row loss
        lse = torch.logsumexp(z, -1)
        zy = z.gather(1, y.clamp(0, V - 1).unsqueeze(1)).squeeze(1)
        hard = (1.0 - smoothing) * (lse - zy) + smoothing * (lse - z.mean(-1))
        out["hard_rows"] = torch.where(good, hard, torch.full_like(hard, float("nan")))
        out["lse"][:, 0] = lse
        h = torch.full((P, V), smoothing / V, dtype=torch.float64)
        for p in range(P):
            if bool(good[p]):
                h[p, int(y[p])] += 1.0 - smoothing
        grad += (1.0 - alpha) * (torch.softmax(z, -1) - h)
    if alpha != 0.0:                                                              # the soft term: KL(q || softmax(z inv_tau))
        logq, c, lses = combined_log_q(teachers, weights, combine, inv_tau)
        s = torch.log_softmax(z * inv_tau, -1)
        q = logq.exp()
        out["soft_rows"] = torch.where(q > 0, q * (logq - s), torch.zeros_like(q)).sum(-1)
        out["lse"][:, 1] = torch.logsumexp(z * inv_tau, -1)
        for i, l in enumerate(lses):
            if l is not None:
                out["tlse"][:, i] = l
        out["cnorm"] = torch.logsumexp(c, -1)
        grad += alpha * tau * (s.exp() - q)
    out["hard"], out["soft"] = out["hard_rows"].mean(), out["soft_rows"].mean()
    out["loss"] = (0.0 if alpha == 1.0 else (1.0 - alpha) * out["hard"]) + (0.0 if alpha == 0.0 else alpha * tau * tau * out["soft"])
    out["accuracy"] = (z.argmax(-1) == y).double().mean()
    out["grad"] = grad * (g / P)
    return out
