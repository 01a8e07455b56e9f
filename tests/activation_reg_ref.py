"""float64 specification of the activation regularisers ("Activation regularisation"; Merity et al. 2017) over ragged captions.

``hidden`` (T1, N, n), time-major: ``hidden[t, i]`` is the top-layer LSTM state of caption ``i`` after decode step ``t``, live while
``t < lengths[i]``; a row that is not live takes no part, whatever it holds.

    P = sum_i len_i        Q = sum_i max(len_i - 1, 0)
    ar  = 1/(P n) sum_i sum_{t < len_i}      |h[t, i]|^2                 (0 when P = 0)
    tar = 1/(Q n) sum_i sum_{1 <= t < len_i} |h[t, i] - h[t-1, i]|^2     (0 when Q = 0)

``decode_train_hidden`` restates the loop of ``oracle.sat_oracle.decode_train`` from that module's own primitives and also returns the
top-layer state after every step; tests/test_activation_reg.py pins it to the oracle's outputs."""
import torch

from oracle import sat_oracle as O


def live_mask(lengths, T1):
    """(T1, N) bool: step t of caption i is live"""
    lens = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1)
    return torch.arange(T1).unsqueeze(1) < lens.unsqueeze(0)


def reg_terms(hidden, lengths):
    """(ar, tar, P, Q) straight from the definitions; ar / tar are 0-dim tensors of hidden's dtype, differentiable in ``hidden``"""
    T1, N, n = hidden.shape
    lens = [int(x) for x in torch.as_tensor(lengths).reshape(-1).tolist()]
    P = sum(lens)
    Q = sum(max(l - 1, 0) for l in lens)
    s0 = hidden.new_zeros(())
    s1 = hidden.new_zeros(())
    for i, l in enumerate(lens):
        for t in range(l):
            s0 = s0 + (hidden[t, i] ** 2).sum()
            if t >= 1:
                s1 = s1 + ((hidden[t, i] - hidden[t - 1, i]) ** 2).sum()
    ar = s0 / (P * n) if P > 0 else hidden.new_zeros(())
    tar = s1 / (Q * n) if Q > 0 else hidden.new_zeros(())
    return ar, tar, P, Q


def reg_grad(hidden, lengths, g0, g1):
    """the closed form of d (g0 ar + g1 tar) / d hidden: zero outside the live rows.  A term that is off is skipped, never multiplied by
    zero, so rows that are not live may hold NaN."""
    T1, N, n = hidden.shape
    lens = [int(x) for x in torch.as_tensor(lengths).reshape(-1).tolist()]
    P = sum(lens)
    Q = sum(max(l - 1, 0) for l in lens)
    out = torch.zeros_like(hidden)
    for i, l in enumerate(lens):
        for t in range(l):
            v = g0 * 2.0 / (P * n) * hidden[t, i]
            if t >= 1:
                v = v + g1 * 2.0 / (Q * n) * (hidden[t, i] - hidden[t - 1, i])
            if t + 1 < l:
                v = v - g1 * 2.0 / (Q * n) * (hidden[t + 1, i] - hidden[t, i])
            out[t, i] = v
    return out


def reg_grad_magnitude(hidden, lengths, g0, g1):
    """|a h_t| + |b| (2 |h_t| + |h_{t-1}| + |h_{t+1}|) per element with only the terms that are on (a = g0 2/(P n), b = g1 2/(Q n)):
    what the rounding error of the closed form scales with.  Zero outside the live rows."""
    T1, N, n = hidden.shape
    lens = [int(x) for x in torch.as_tensor(lengths).reshape(-1).tolist()]
    P = sum(lens)
    Q = sum(max(l - 1, 0) for l in lens)
    out = torch.zeros_like(hidden)
    for i, l in enumerate(lens):
        for t in range(l):
            v = abs(g0 * 2.0 / (P * n)) * hidden[t, i].abs()
            if t >= 1:
                v = v + abs(g1 * 2.0 / (Q * n)) * (hidden[t, i].abs() + hidden[t - 1, i].abs())
            if t + 1 < l:
                v = v + abs(g1 * 2.0 / (Q * n)) * (hidden[t + 1, i].abs() + hidden[t, i].abs())
            out[t, i] = v
    return out


def decode_train_hidden(sd, hp, ann_img, caps, lengths, epsilon=0, draw=None):
    """``O.decode_train`` (no dropout masks) with one more output: ``hidden`` (T-1, N, n), the top-layer state after each step (rows of
    finished captions keep their last state, as ``h`` does in the loop)."""
    if draw is None:
        draw = lambda: float(torch.rand(1))
    layers, n, V = hp.decoder_layers, hp.decoder_dim, hp.vocab_size
    R = lengths.size(1)
    ann = ann_img.repeat_interleave(R, dim=0)
    _, _, Hh, Ww = ann.shape
    caps = caps.reshape(-1, caps.size(2))
    lens = lengths.reshape(-1)
    h, c = O.init_state(sd, ann, layers, n, None)
    h, c = h.clone(), c.clone()
    N, T = caps.shape
    logits = torch.zeros(N, T - 1, V)
    alphas = torch.zeros(N, T - 1, Hh * Ww)
    hidden = []
    for step in range(T - 1):
        live = lens > step
        if not bool(live.any()):
            break
        if step <= 2 or draw() <= epsilon:
            tok = caps[live, step]
        else:
            tok = torch.argmax(logits[live, step - 1, :], dim=1)
        y = O.embed(sd, tok, getattr(hp, "embed_norm", None))
        z, alpha = O.soft_attention(sd, ann[live], h[-1, live])
        alphas[live, step, :] = alpha.reshape(int(live.sum()), Hh * Ww)
        gate = O.beta_gate(sd, h[-1, live])
        x = torch.cat([y, gate * z], dim=1).unsqueeze(0)
        hn, cn = O.lstm_step(sd, x, h[:, live], c[:, live], layers)
        h = h.clone(); c = c.clone()
        h[:, live] = hn
        c[:, live] = cn
        hidden.append(h[-1])
        logits[live, step, :] = O.deep_output(sd, y, h[-1, live], z, hp.deep_output, None).float()
    while len(hidden) < T - 1:          # steps no caption reaches: never live
        hidden.append(torch.zeros(N, n))
    return dict(logits=logits, alphas=alphas, targets=caps[:, 1:], lengths=lens, hidden=torch.stack(hidden))


def training_loss_reg(sd, hp, ann_img, caps, lengths, ar_alpha, tar_beta, epsilon=0, draw=None):
    """``O.training_loss`` plus ``ar_alpha * ar + tar_beta * tar`` of the top-layer states: (loss, parts with "ar" / "tar" / "base")"""
    out = decode_train_hidden(sd, hp, ann_img, caps, lengths, epsilon, draw)
    lp, _ = O.pack_time_major(out["logits"], out["lengths"])
    tp, _ = O.pack_time_major(out["targets"], out["lengths"])
    base = O.label_smoothing_ce(lp, tp, hp.label_smoothing) + O.doubly_stochastic(out["alphas"], hp.att_gamma)
    ar, tar, P, Q = reg_terms(out["hidden"].double(), out["lengths"])          # the sums in float64; autograd goes through the cast
    out.update(base=base.detach(), ar=ar.detach(), tar=tar.detach(), P=P, Q=Q)
    return base + (ar_alpha * ar + tar_beta * tar).float(), out
