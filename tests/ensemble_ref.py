"""CPU reference of ensemble decoding ("Ensemble decoding"): the combination of several models' per-step distributions
restated in float64, and ``history_ref.beam_search`` over a list of members.  Plain torch on the host plus the oracle's own decoder
pieces; nothing shared with the kernels.

Members i = 0 .. M - 1, weights w_i >= 0 summing to 1, temperature T, l_i = log_softmax(z_i / T):
  arithmetic  c_v = log sum_i w_i exp(l_i,v)      (a mixture of the distributions)
  geometric   c_v = sum_i w_i l_i,v               (a product of experts)
members with w_i == 0 are skipped; the step's score is parent + log_softmax(c)_v, then the masks and rules of the plain search."""
import math

import torch
import torch.nn.functional as F

from oracle import sat_oracle as O

from history_ref import _boundary_gap, blocked_words


def combine(logits_list, weights, combine, T):
    """c in float64 for logits of any shape (..., V), one tensor per member"""
    assert combine in ("arithmetic", "geometric") and len(logits_list) == len(weights)
    ls = [F.log_softmax(z.double() / float(T), dim=-1) for z, w in zip(logits_list, weights) if w != 0]
    ws = [float(w) for w in weights if w != 0]
    if combine == "geometric":
        return sum(w * l for w, l in zip(ws, ls))
    return torch.logsumexp(torch.stack([l + math.log(w) for w, l in zip(ws, ls)]), dim=0)


def beam_search(members, weights, combine_mode, beamk=3, max_gen_length=32, temperature=1.0, rescore_method=None, rescore_reward=0.5, return_all=False,
                no_repeat_ngram=0, min_length=0, banned=(), margins=None):
    """``history_ref.beam_search`` ("beam" sampling, no penalty) over ``members``, a list of ``(sd, hp, ann_img)``: the oracle's functions
    per member, one shared selection.  The returned maps are member 0's.  ``margins`` as in ``history_ref``."""
    hp0 = members[0][1]
    stoi = hp0.vocab_stoi
    START, PAD, END, UNK = int(stoi["<START>"]), int(stoi["<PAD>"]), int(stoi["<END>"]), int(stoi["<UNK>"])
    V = hp0.vocab_size
    temps = temperature if isinstance(temperature, list) else [temperature]
    ngram = int(no_repeat_ngram)
    banned = sorted(set(int(t) for t in banned))
    M = len(members)
    if margins is not None:
        margins.setdefault("boundary", []); margins.setdefault("final", [])
    captions, cap_scores, cap_alphas, cap_ppl = [], [], [], []
    _, _, Hh, Ww = members[0][2].shape
    for idx in range(members[0][2].shape[0]):
        k = beamk
        annots = [ann[idx].expand(k, *ann[idx].shape) for _, _, ann in members]
        states = [O.init_state(sd, annots[i], hp.decoder_layers, hp.decoder_dim) for i, (sd, hp, _) in enumerate(members)]
        hs, cs = [s[0] for s in states], [s[1] for s in states]
        top_preds = torch.full((1, k), START, dtype=torch.long)
        top_scores = torch.zeros(k)
        alphas = torch.zeros(1, k, Hh, Ww)
        fin_caps, fin_alphas, fin_scores, fin_ppl = [], [], [], []

        def rescore(s, step):
            if rescore_method == "LN":
                return s / step
            if rescore_method == "WR":
                return s + rescore_reward * step
            if rescore_method == "BAR":
                return s + rescore_reward * (-torch.mean(top_scores))
            return s

        step = 0
        while True:
            T = temps[step % len(temps)]
            logits, alpha = [], None
            for i, (sd, hp, _) in enumerate(members):
                y = O.embed(sd, top_preds[step])
                z, a = O.soft_attention(sd, annots[i], hs[i][-1])
                x = torch.cat([y, O.beta_gate(sd, hs[i][-1]) * z], dim=1).unsqueeze(0)
                hs[i], cs[i] = O.lstm_step(sd, x, hs[i], cs[i], hp.decoder_layers)
                logits.append(O.deep_output(sd, y, hs[i][-1], z, hp.deep_output))
                if i == 0:
                    alpha = a
            hists = [top_preds[1:step + 1, i].tolist() for i in range(k)]
            scores = F.log_softmax(combine(logits, weights, combine_mode, T), dim=1).float()
            scores[:, [START, PAD] + banned] = float("-inf")
            if step == 0:
                scores[:, [END, UNK]] = float("-inf")
            if step < min_length:
                scores[:, END] = float("-inf")
            if ngram >= 1:
                for i in range(k):
                    for v in blocked_words(hists[i], ngram):
                        scores[i, v] = float("-inf")
            if step == 0:
                if margins is not None:
                    margins["boundary"].append(_boundary_gap(scores[0], k))
                top_scores, pred_idx = torch.topk(scores[0], k)
                top_preds = torch.cat([top_preds, pred_idx.unsqueeze(0)], 0)
                alphas = torch.cat([alphas, alpha.unsqueeze(0)], 0)
            else:
                seq = scores + top_scores.unsqueeze(1)
                if margins is not None:
                    margins["boundary"].append(_boundary_gap(seq.reshape(-1), k))
                _, pred_idx = torch.topk(seq.reshape(-1), k, dim=0)
                top_scores = seq.reshape(-1)[pred_idx]
                keep = torch.div(pred_idx, V, rounding_mode="floor")
                word = torch.remainder(pred_idx, V).unsqueeze(0)
                top_preds = torch.cat([top_preds[:, keep], word], 0)
                alphas = torch.cat([alphas[:, keep], alpha.unsqueeze(0)[:, keep]], 0)
                for i in range(M):
                    hs[i], cs[i], annots[i] = hs[i][:, keep], cs[i][:, keep], annots[i][keep]
            complete = top_preds[step + 1] == END
            if bool(complete.any()):
                for i in torch.nonzero(complete).flatten().tolist():
                    fin_caps.append(top_preds[:, i][1:-1].tolist())
                    fin_alphas.append(alphas[:, i][1:-1].clone())
                    fin_scores.append(float(rescore(top_scores[i], step)))
                    fin_ppl.append(float(torch.exp(-top_scores[i] / step)))
                inc = ~complete
                top_preds, alphas, top_scores = top_preds[:, inc], alphas[:, inc], top_scores[inc]
                for i in range(M):
                    hs[i], cs[i], annots[i] = hs[i][:, inc], cs[i][:, inc], annots[i][inc]
                k = int(inc.sum())
                if k == 0:
                    break
            if step >= max_gen_length:
                for i in range(top_preds.shape[1]):
                    fin_caps.append(top_preds[:, i][1:-1].tolist())
                    fin_alphas.append(alphas[:, i][1:-1].clone())
                    fin_scores.append(float(rescore(top_scores[i], step)))
                    fin_ppl.append(float(torch.exp(-top_scores[i] / step)))
                break
            step += 1
        if margins is not None:
            s = sorted(fin_scores, reverse=True)
            margins["final"].append([a - b for a, b in zip(s, s[1:])])
        if return_all:
            order = [i for _, i in sorted([[fin_scores[i], i] for i in range(len(fin_scores))], reverse=True)]
            captions.append([fin_caps[i] for i in order]); cap_alphas.append([fin_alphas[i] for i in order])
            cap_scores.append([fin_scores[i] for i in order]); cap_ppl.append([fin_ppl[i] for i in order])
        else:
            best = fin_scores.index(max(fin_scores))
            captions.append(fin_caps[best]); cap_alphas.append(fin_alphas[best])
            cap_scores.append(fin_scores[best]); cap_ppl.append(fin_ppl[best])
    return captions, cap_scores, cap_alphas, cap_ppl
