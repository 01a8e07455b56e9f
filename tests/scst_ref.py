"""The specification of self-critical training (include/sat_hip.h: sat_policy_nll_fwd / _bwd, sat_scst_prepare, SAT_SAMPLE_ANCESTRAL)
restated in float64 torch / numpy: the row-weighted policy loss over the unmasked words, its gradient, the train batch built from the
scores of sampled captions, and one ancestral draw."""
import numpy as np
import torch

GREEDY, MEAN = 0, 1


def unmasked(P, V, masked_ids, n_first_rows):
    """bool (P, V): the words row p may draw.  The first n_first_rows rows mask all four ids, the others the first two; an id outside
    [0, V) masks nothing."""
    keep = torch.ones(P, V, dtype=torch.bool)
    for p in range(P):
        for m in list(masked_ids)[:4 if p < n_first_rows else 2]:
            if 0 <= int(m) < V:
                keep[p, int(m)] = False
    return keep


def policy_loss(logits, targets, row_weight, inv_temperature, masked_ids, n_first_rows, scale):
    """(loss, logq (P), lse (P)) in the dtype of ``logits`` (pass float64).  Differentiable in ``logits``.  A row of weight zero adds
    exactly 0; a target outside [0, V) or masked in its row gives a NaN logq (and a NaN loss when its weight is not zero)."""
    P, V = logits.shape
    keep = unmasked(P, V, masked_ids, n_first_rows)
    x = logits * inv_temperature
    lse = torch.logsumexp(x.masked_fill(~keep, -float("inf")), dim=1)
    t = torch.as_tensor(targets).to(torch.int64)
    valid = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)
    valid = valid & keep[torch.arange(P), tc]
    logq = x[torch.arange(P), tc] - lse
    logq = torch.where(valid, logq, torch.full_like(logq, float("nan")))
    w = torch.as_tensor(row_weight).to(logits.dtype)
    terms = torch.where(w != 0, w * logq, torch.zeros_like(logq))
    return -scale * terms.sum(), logq, lse


def policy_grad(logits, targets, row_weight, inv_temperature, masked_ids, n_first_rows, scale, g=1.0):
    """the closed form of d loss / d logits: g * scale * w_p * inv_temperature * (softmax_U(x) - onehot(target)) on the unmasked words, 0 on
    the masked ones and in the rows of weight zero"""
    P, V = logits.shape
    keep = unmasked(P, V, masked_ids, n_first_rows)
    x = (logits * inv_temperature).masked_fill(~keep, -float("inf"))
    sm = torch.softmax(x, dim=1)
    t = torch.as_tensor(targets).to(torch.int64)
    onehot = torch.zeros_like(sm)
    for p in range(P):
        if 0 <= int(t[p]) < V and keep[p, int(t[p])]:
            onehot[p, int(t[p])] = 1.0
    w = torch.as_tensor(row_weight).to(logits.dtype)
    grad = g * scale * inv_temperature * w[:, None] * (sm - onehot)
    grad = torch.where(keep, grad, torch.zeros_like(grad))
    return torch.where((w != 0)[:, None], grad, torch.zeros_like(grad))


def prepare(cap_tokens, cap_len, scores, scores_greedy, K, w_cider, w_rouge, mode, ids):
    """numpy restatement of sat_scst_prepare.  cap_tokens (N, S + 1), cap_len (N), scores (N, 2) float64, scores_greedy (B, 2) or None,
    ids = (START, PAD, END, UNK).  Returns dict(reward, baseline, advantage float32 (N); caps (N, S + 2) int32; lengths (N) int32;
    step_weight (N, S + 1) float32; count (N) int32)."""
    cap_tokens, cap_len = np.asarray(cap_tokens), np.asarray(cap_len)
    scores = np.asarray(scores, np.float64)
    N, W = cap_tokens.shape
    S, T = W - 1, W + 1
    B = N // K
    START, PAD, END, _ = [int(i) for i in ids]
    r = w_cider * scores[:, 0] + w_rouge * scores[:, 1]
    base = np.zeros(N, np.float64)
    for n in range(N):
        b, k = divmod(n, K)
        if mode == GREEDY:
            sg = np.asarray(scores_greedy, np.float64)
            base[n] = w_cider * sg[b, 0] + w_rouge * sg[b, 1]
        else:
            s = 0.0
            for j in range(K):
                if j != k:
                    s += r[b * K + j]
            base[n] = s / (K - 1)
    adv = (r - base).astype(np.float32)
    caps = np.full((N, T), PAD, np.int32)
    lengths, count = np.zeros(N, np.int32), np.zeros(N, np.int32)
    sw = np.zeros((N, T - 1), np.float32)
    for n in range(N):
        ln = min(max(int(cap_len[n]), 1), S)
        caps[n, 0] = START
        caps[n, 1:1 + ln] = cap_tokens[n, :ln]
        caps[n, 1 + ln] = END
        lengths[n] = ln + 1
        sw[n, :ln] = adv[n]
        if ln < S:
            sw[n, ln] = adv[n]
        count[n] = ln + (1 if ln < S else 0)
    return dict(reward=r.astype(np.float32), baseline=base.astype(np.float32), advantage=adv, caps=caps, lengths=lengths, step_weight=sw, count=count)


def masked_log_softmax(logits, temperature, masked_ids):
    """float64 (V): log_softmax(logits / T) with the masked ids at -inf (the search's scores of one step without the running sum)"""
    s = torch.log_softmax(torch.as_tensor(logits, dtype=torch.float64) / temperature, dim=-1).clone()
    for m in masked_ids:
        if 0 <= int(m) < s.shape[-1]:
            s[..., int(m)] = -float("inf")
    return s


def ancestral_draw(logits, temperature, masked_ids, gumbel):
    """(word, gap): arg-max of masked log_softmax(logits / T) + G, ties to the lower id, and the distance of the runner-up key"""
    key = masked_log_softmax(logits, temperature, masked_ids) + torch.as_tensor(gumbel, dtype=torch.float64)
    top = torch.topk(key, 2)
    word = int(torch.nonzero(key == top.values[0])[0])
    return word, float(top.values[0] - top.values[1])
