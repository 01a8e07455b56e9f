"""float64 specification of the token losses (include/sat_hip.h, sat_token_loss_fwd / _bwd; DESIGN.md 5, "Token losses"), definition by
definition: the label-smoothed cross entropy, focal loss (Lin et al. 2017) and token-level unlikelihood (Welleck et al. 2019) over packed
rows.  The candidate sets are built by brute force from (captions, lengths) in packed order, the loss goes through ``torch.log_softmax``
and ``clamp``, the gradient comes from autograd; ``closed_form_grad`` is the formula the kernels implement, checked against autograd in
tests/test_token_loss.py.  A term whose weight is 0 is skipped and reported as 0, as the kernels do.

``training_loss_token`` restates the oracle's step loss with the new terms on the oracle's own packed logits."""
import torch

from oracle import sat_oracle as O

CLAMP = 1e-5
TOKEN_LOSSES = {"ce": (1.0, 0.0), "fl": (0.0, 1.0), "ce+fl": (1.0, 1.0)}


def packed_steps(lengths, T):
    """(caption index, decode step) of every packed row, in the order of ``pack_padded_sequence`` (the oracle's ``pack_time_major``)"""
    lens = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1)
    N = lens.numel()
    idx = torch.arange(N * (T - 1)).view(N, T - 1)
    rows, _ = O.pack_time_major(idx, lens)
    return rows // (T - 1), rows % (T - 1)


def src_rows(lengths, T):
    """src_row[p] = t * N + i: what ``PackPlan.src_row`` holds for the same lengths (up to the order of captions of equal length)"""
    cap, step = packed_steps(lengths, T)
    return (step * torch.as_tensor(lengths).numel() + cap).to(torch.int32)


def candidates(caps2, lengths, V, pad_id):
    """per packed row (caption i, step t): the sorted distinct ids among caps2[i][1 .. t] that are not the row's target caps2[i][t + 1],
    not ``pad_id`` and inside [0, V); also the rows' targets"""
    N, T = caps2.shape
    cap, step = packed_steps(lengths, T)
    out, targets = [], []
    for i, t in zip(cap.tolist(), step.tolist()):
        y = int(caps2[i, t + 1])
        seen = set()
        for s in range(1, t + 1):
            c = int(caps2[i, s])
            if c != y and c != pad_id and 0 <= c < V:
                seen.add(c)
        out.append(sorted(seen))
        targets.append(y)
    return out, torch.tensor(targets, dtype=torch.int64)


def row_terms(z, y, cand, smoothing, gamma, with_fl=True, with_ul=True):
    """(ce, fl, ul, mass) rows in z's dtype, differentiable in z; ``logp`` comes back too"""
    P, V = z.shape
    logp = torch.log_softmax(z, dim=-1)
    nll = -logp.gather(1, y.view(-1, 1)).squeeze(1)
    ce = (1.0 - smoothing) * nll + smoothing * (-logp.mean(dim=-1))
    fl = torch.zeros_like(nll)
    if with_fl:
        fl = nll if gamma == 0 else (-torch.expm1(-nll)) ** gamma * nll
    ul, mass = [], []
    for p in range(P):
        if with_ul and cand[p]:
            lc = logp[p, torch.tensor(cand[p])]
            ul.append(-(-torch.expm1(lc)).clamp(min=CLAMP).log().sum())
            mass.append(lc.exp().sum())
        else:
            ul.append(z.new_zeros(()))
            mass.append(z.new_zeros(()))
    return ce, fl, torch.stack(ul), torch.stack(mass), logp


def token_loss(z, y, cand, smoothing, ce_weight, focal_weight, gamma, ul_alpha, g=1.0):
    """everything sat_token_loss_fwd / _bwd produce, in float64: loss, accuracy, the four means, the rows, lse, and the gradient of
    g * loss from autograd"""
    zd = z.detach().double().clone().requires_grad_()
    y = y.to(torch.int64)
    P, V = zd.shape
    ce, fl, ul, mass, logp = row_terms(zd, y, cand, smoothing, gamma, focal_weight != 0, ul_alpha != 0)
    if ce_weight == 0:
        ce = torch.zeros_like(ce)
    total = zd.new_zeros(())
    for wgt, rows in ((ce_weight, ce), (focal_weight, fl), (ul_alpha, ul)):
        if wgt != 0:
            total = total + wgt * rows.mean()
    (total * g).backward()
    with torch.no_grad():
        om = [float((-torch.expm1(logp[p, torch.tensor(c)])).min()) for p, c in enumerate(cand) if c and ul_alpha != 0]
        return dict(loss=total.detach(), accuracy=(zd.argmax(dim=1) == y).double().mean(), ce=ce.mean().detach(), fl=fl.mean().detach(),
                    ul=ul.mean().detach(), mass=mass.mean().detach(), rows=torch.stack([ce, fl, ul, mass], dim=1).detach(),
                    lse=torch.logsumexp(zd, dim=1).detach(), grad=zd.grad.clone(), min_one_minus_p=min(om) if om else 1.0)


def closed_form_grad(z, y, cand, smoothing, ce_weight, focal_weight, gamma, ul_alpha, g=1.0):
    """the gradient as include/sat_hip.h states it, float64, row by row; returns (grad, w rows, R rows)"""
    zd = z.detach().double()
    P, V = zd.shape
    prob = torch.softmax(zd, dim=-1)
    logp = torch.log_softmax(zd, dim=-1)
    grad = torch.zeros_like(zd)
    ws, Rs = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
    for p in range(P):
        t = int(y[p])
        row = torch.zeros(V, dtype=torch.float64)
        onehot = torch.zeros(V, dtype=torch.float64); onehot[t] = 1.0
        if ce_weight != 0:
            row += ce_weight * (prob[p] - smoothing / V - (1.0 - smoothing) * onehot)
        if focal_weight != 0:
            logq = logp[p, t]
            q, om = torch.exp(logq), -torch.expm1(logq)
            if gamma == 0:
                w = torch.ones((), dtype=torch.float64)
            elif float(om) == 0.0:
                w = torch.zeros((), dtype=torch.float64)
            else:
                w = om ** gamma - gamma * q * om ** (gamma - 1.0) * logq
            ws[p] = w
            row += focal_weight * w * (prob[p] - onehot)
        if ul_alpha != 0 and cand[p]:
            c = torch.tensor(cand[p])
            pc, om = prob[p, c], -torch.expm1(logp[p, c])
            r = torch.where(om >= CLAMP, pc / om, torch.zeros_like(pc))
            Rs[p] = r.sum()
            row += ul_alpha * (-prob[p] * r.sum())
            row[c] += ul_alpha * r
        grad[p] = row * (g / P)
    return grad, ws, Rs


def training_loss_token(sd, hp, ann_img, caps, lengths, token_loss="ce", focal_gamma=2.0, ul_alpha=0.0, epsilon=0, draw=None, pad_id=0):
    """``O.training_loss`` with the token loss in the cross entropy's place, on the oracle's own packed logits: (loss, parts with "ce" /
    "fl" / "ul" / "repeat_mass" / "base", the unweighted means and the loss without the new terms).  The candidates come from the
    ground-truth captions whatever word was fed back."""
    ce_weight, focal_weight = TOKEN_LOSSES[token_loss]
    out = O.decode_train(sd, hp, ann_img, caps, lengths, epsilon, draw)
    lp, bs = O.pack_time_major(out["logits"], out["lengths"])
    tp, _ = O.pack_time_major(out["targets"], out["lengths"])
    ds = O.doubly_stochastic(out["alphas"], hp.att_gamma)
    base = O.label_smoothing_ce(lp, tp, hp.label_smoothing) + ds
    if token_loss == "ce" and ul_alpha == 0:
        out.update(logits_packed=lp, targets_packed=tp, batch_sizes=bs, base=base.detach(), loss=base)
        return base, out
    caps2 = caps.reshape(-1, caps.size(2))
    cand, y = candidates(caps2, out["lengths"], hp.vocab_size, pad_id)
    assert torch.equal(y, tp)
    ce, fl, ul, mass, _ = row_terms(lp.double(), tp, cand, hp.label_smoothing, focal_gamma, focal_weight != 0, ul_alpha != 0)      # float64; autograd goes through the cast
    if ce_weight == 0:
        ce = torch.zeros_like(ce)
    total = lp.new_zeros((), dtype=torch.float64)
    for wgt, rows in ((ce_weight, ce), (focal_weight, fl), (ul_alpha, ul)):
        if wgt != 0:
            total = total + wgt * rows.mean()
    loss = total.float() + ds
    pred = torch.argmax(lp, dim=1)
    out.update(logits_packed=lp, targets_packed=tp, batch_sizes=bs, base=base.detach(), loss=loss, ce=ce.mean().detach(), fl=fl.mean().detach(),
               ul=ul.mean().detach(), repeat_mass=mass.mean().detach(), acc=torch.sum(pred == tp) / pred.shape[0], candidates=cand)
    return loss, out
