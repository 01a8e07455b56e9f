"""Specification of the layer-normalised LSTM cell ("Layer-normalised LSTM"; Ba et al. 2016, the single-matmul form).

Per layer ``l``, with the pre-activation ``a = x W_ih^T + b_ih + h W_hh^T + b_hh`` (gate order i, f, g, o; width 4n):

    a^_k = LN(a_k; gamma_k, beta_k)          k in {i, f, g, o}, each over its own n units
    i = s(a^_i)  f = s(a^_f)  g = tanh(a^_g)  o = s(a^_o)
    c_t = f c_{t-1} + i g                    (carried un-normalised)
    h_t = o tanh(LN(c_t; gamma_c, beta_c))

``LN`` is ``torch.nn.functional.layer_norm`` (biased variance) with eps = 1e-5.  The parameters live in the state dict under
``lstm_ln.gates_l{l}.weight`` / ``.bias`` (4n) and ``lstm_ln.cell_l{l}.weight`` / ``.bias`` (n).  Everything works in the dtype it is
given.  ``ln_lstm_step`` has the signature of ``oracle.sat_oracle.lstm_step``, so it goes into ``O.decode_train(lstm_fn=)`` and
``O.beam_search(lstm_fn=)`` as it is."""
import torch
import torch.nn.functional as F

from oracle import prng, sat_oracle as O

EPS = 1e-5


def ln_keys(layers):
    return ["lstm_ln.%s_l%d.%s" % (mod, l, par) for l in range(layers) for mod in ("gates", "cell") for par in ("weight", "bias")]


def ln_state(n, layers, seed):
    """random layer-norm parameters: gains in [0.5, 1.5], shifts in [-0.5, 0.5], so that a dropped gain or shift cannot pass"""
    sd = {}
    for i, k in enumerate(ln_keys(layers)):
        width = 4 * n if ".gates_" in k else n
        lo, hi = (0.5, 1.5) if k.endswith("weight") else (-0.5, 0.5)
        sd[k] = torch.from_numpy(prng.uniform((width,), seed + i, lo, hi))
    return sd


def _ln(x, w, b):
    """layer norm over the last dimension written out: biased variance, eps inside the root"""
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * w + b


def ln_cell(a, c_prev, gw, gb, cw, cb):
    """the pointwise part on the summed pre-activation a (N, 4n): dict(gates (activated, N x 4n), c, h, xhat (N, 5n), rstd (N, 5))"""
    n = c_prev.shape[-1]
    acts, xhat, rstd = [], [], []
    for k in range(4):
        ak = a[..., k * n:(k + 1) * n]
        mu = ak.mean(dim=-1, keepdim=True)
        r = 1.0 / torch.sqrt(((ak - mu) ** 2).mean(dim=-1, keepdim=True) + EPS)
        xh = (ak - mu) * r
        xhat.append(xh); rstd.append(r)
        v = xh * gw[k * n:(k + 1) * n] + gb[k * n:(k + 1) * n]
        acts.append(torch.tanh(v) if k == 2 else torch.sigmoid(v))
    i, f, g, o = acts
    c = f * c_prev + i * g
    mu = c.mean(dim=-1, keepdim=True)
    r = 1.0 / torch.sqrt(((c - mu) ** 2).mean(dim=-1, keepdim=True) + EPS)
    ch = (c - mu) * r
    xhat.append(ch); rstd.append(r)
    h = o * torch.tanh(ch * cw + cb)
    return dict(gates=torch.cat(acts, dim=-1), c=c, h=h, xhat=torch.cat(xhat, dim=-1), rstd=torch.cat(rstd, dim=-1))


def ln_lstm_step(sd, x, h, c, layers):
    """one time step of the stacked layer-normalised LSTM.  x (1, N, in); h, c (layers, N, n) -> (h, c) new"""
    hs, cs = [], []
    inp = x[0]
    for l in range(layers):
        a = (F.linear(inp, sd["lstm.weight_ih_l%d" % l], sd["lstm.bias_ih_l%d" % l])
             + F.linear(h[l], sd["lstm.weight_hh_l%d" % l], sd["lstm.bias_hh_l%d" % l]))
        out = ln_cell(a, c[l], sd["lstm_ln.gates_l%d.weight" % l], sd["lstm_ln.gates_l%d.bias" % l],
                      sd["lstm_ln.cell_l%d.weight" % l], sd["lstm_ln.cell_l%d.bias" % l])
        hs.append(out["h"]); cs.append(out["c"])
        inp = out["h"]
    return torch.stack(hs), torch.stack(cs)


def ln_lstm_step_layer_norm(sd, x, h, c, layers):
    """the same step composed from ``F.layer_norm`` (tests pin ``ln_lstm_step`` to it)"""
    hs, cs = [], []
    inp = x[0]
    for l in range(layers):
        n = h.shape[-1]
        a = (F.linear(inp, sd["lstm.weight_ih_l%d" % l], sd["lstm.bias_ih_l%d" % l])
             + F.linear(h[l], sd["lstm.weight_hh_l%d" % l], sd["lstm.bias_hh_l%d" % l]))
        gw, gb = sd["lstm_ln.gates_l%d.weight" % l], sd["lstm_ln.gates_l%d.bias" % l]
        v = [F.layer_norm(a[:, k * n:(k + 1) * n], (n,), gw[k * n:(k + 1) * n], gb[k * n:(k + 1) * n], EPS) for k in range(4)]
        cn = torch.sigmoid(v[1]) * c[l] + torch.sigmoid(v[0]) * torch.tanh(v[2])
        hn = torch.sigmoid(v[3]) * torch.tanh(F.layer_norm(cn, (n,), sd["lstm_ln.cell_l%d.weight" % l], sd["lstm_ln.cell_l%d.bias" % l], EPS))
        hs.append(hn); cs.append(cn)
        inp = hn
    return torch.stack(hs), torch.stack(cs)


def training_loss_ln(sd, hp, ann_img, caps, lengths, epsilon=0, draw=None, masks=None, lstm_fn=ln_lstm_step):
    """``O.training_loss`` with the normalised cell: (loss, parts with "logits_packed")"""
    out = O.decode_train(sd, hp, ann_img, caps, lengths, epsilon, draw, lstm_fn=lstm_fn, masks=masks)
    lp, _ = O.pack_time_major(out["logits"], out["lengths"])
    tp, _ = O.pack_time_major(out["targets"], out["lengths"])
    loss = O.label_smoothing_ce(lp, tp, hp.label_smoothing) + O.doubly_stochastic(out["alphas"], hp.att_gamma)
    out.update(logits_packed=lp, targets_packed=tp, loss=loss)
    return loss, out
