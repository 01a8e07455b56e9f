"""CPU reference of the diverse (group) beam search ("Diverse beam search"): the whole search restated in torch fp32 on
the oracle's decoder pieces, after ``history_ref.beam_search``.  No GPU, nothing shared with the kernels.

A beam of K rows is G groups of Kg = K / G rows.  A group is a beam search of its own (its own rows, parents, finished list and cut);
the groups of an image advance in lockstep and at every step select one after the other, g = 0 .. G - 1.  Group g ranks its candidates
(row j, word v) by pen = s[j, v] - lambda * c[v] in fp32, product first, c[v] = how many hypotheses the groups before it kept with word
v at this step (<END> included; a group that has ended adds nothing), descending with ties to the lower flat index j * V + v.  The
hypothesis carries s, never pen.  The finished list of an image is its groups' lists one after the other.

Every group runs the very operations of ``history_ref.beam_search`` on its own Kg rows, so G = 1, and every group at lambda = 0, give
that search's floats bit for bit."""
import torch
import torch.nn.functional as F

import history_ref as HR
from oracle import sat_oracle as O


def decode_step(sd, hp, annots, h, c, tokens):
    """one step of the decoder for the rows of ``annots``: (raw logits, attention maps, h, c); the operations of history_ref"""
    y = O.embed(sd, tokens)
    z, alpha = O.soft_attention(sd, annots, h[-1])
    x = torch.cat([y, O.beta_gate(sd, h[-1]) * z], dim=1).unsqueeze(0)
    h, c = O.lstm_step(sd, x, h, c, hp.decoder_layers)
    return O.deep_output(sd, y, h[-1], z, hp.deep_output), alpha, h, c


def sequence_logprob(sd, hp, ann_one, words, temperature=1.0):
    """the sum of log-softmax(logits / T_s)[words[s]] over s, teacher-forcing <START>, words[0], words[1], ... through ``decode_step`` for
    one image ``ann_one`` (D, H, W): what a hypothesis that said ``words`` (its closing <END> or cut word included) scores"""
    temps = temperature if isinstance(temperature, list) else [temperature]
    annots = ann_one.unsqueeze(0)
    h, c = O.init_state(sd, annots, hp.decoder_layers, hp.decoder_dim)
    fed, total = int(hp.vocab_stoi["<START>"]), torch.zeros(())
    for s, w in enumerate(words):
        logits, _, h, c = decode_step(sd, hp, annots, h, c, torch.tensor([fed]))
        total = total + F.log_softmax(logits / temps[s % len(temps)], dim=1)[0, int(w)]
        fed = int(w)
    return float(total)


class _Group:
    """the state of one group of one image: history_ref.beam_search's locals"""

    def __init__(self, sd, hp, ann_one, k, start):
        self.k = k
        self.annots = ann_one.expand(k, *ann_one.shape)
        self.h, self.c = O.init_state(sd, self.annots, hp.decoder_layers, hp.decoder_dim)
        self.top_preds = torch.full((1, k), start, dtype=torch.long)
        self.top_scores = torch.zeros(k)
        self.alphas = torch.zeros(1, k, *ann_one.shape[1:])
        self.caps, self.fin_alphas, self.scores, self.ppl = [], [], [], []
        self.done = False


def beam_search(sd, hp, ann_img, beamk=4, beam_groups=1, diversity_penalty=0.5, max_gen_length=32, temperature=1.0, rescore_method=None,
                rescore_reward=0.5, return_all=False, no_repeat_ngram=0, min_length=0, repetition_penalty=1.0, banned=(), margins=None,
                trace=None):
    """``history_ref.beam_search`` with groups and banned ids.  ``margins`` as there, "boundary" taken on the PENALISED values of each
    group's selection.  ``trace``: a list that receives ``(image, step, group, words kept)`` for every selection."""
    stoi = hp.vocab_stoi
    START, PAD, END, UNK = int(stoi["<START>"]), int(stoi["<PAD>"]), int(stoi["<END>"]), int(stoi["<UNK>"])
    V = hp.vocab_size
    G = max(int(beam_groups or 1), 1)
    assert beamk % G == 0
    Kg = beamk // G
    lam = torch.tensor(float(diversity_penalty), dtype=torch.float32)
    temps = temperature if isinstance(temperature, list) else [temperature]
    ngram, theta, banned = int(no_repeat_ngram), float(repetition_penalty), [int(t) for t in banned]
    if margins is not None:
        margins.setdefault("boundary", []); margins.setdefault("final", [])
    captions, cap_scores, cap_alphas, cap_ppl = [], [], [], []
    for idx in range(ann_img.shape[0]):
        groups = [_Group(sd, hp, ann_img[idx], Kg, START) for _ in range(G)]
        step = 0
        while not all(g.done for g in groups):
            T = temps[step % len(temps)]
            count = torch.zeros(V)                       # c[v]: the words the earlier groups kept at this step
            for gi, g in enumerate(groups):
                if g.done:
                    continue
                k = g.k
                logits, alpha, g.h, g.c = decode_step(sd, hp, g.annots, g.h, g.c, g.top_preds[step])
                hists = [g.top_preds[1:step + 1, i].tolist() for i in range(k)]
                if theta != 1.0 and step > 0:
                    logits = torch.stack([HR.penalise(logits[i], hists[i], theta) for i in range(k)])
                scores = F.log_softmax(logits / T, dim=1)
                scores[:, [START, PAD]] = float("-inf")
                if step == 0:
                    scores[:, [END, UNK]] = float("-inf")
                if banned:
                    scores[:, banned] = float("-inf")
                if step < min_length:
                    scores[:, END] = float("-inf")
                if ngram >= 1:
                    for i in range(k):
                        for v in HR.blocked_words(hists[i], ngram):
                            scores[i, v] = float("-inf")
                seq = scores[0] if step == 0 else (scores + g.top_scores.unsqueeze(1)).reshape(-1)
                pen = seq - (lam * count).repeat(seq.numel() // V)          # two fp32 roundings: the product, then the difference
                if margins is not None:
                    margins["boundary"].append(HR._boundary_gap(pen, k))
                pred_idx = torch.sort(pen, descending=True, stable=True).indices[:k]   # ties to the lower flat index
                g.top_scores = seq[pred_idx]                                # the hypothesis carries s, not pen
                if step == 0:
                    g.top_preds = torch.cat([g.top_preds, pred_idx.unsqueeze(0)], 0)
                    g.alphas = torch.cat([g.alphas, alpha.unsqueeze(0)], 0)
                else:
                    keep = torch.div(pred_idx, V, rounding_mode="floor")
                    word = torch.remainder(pred_idx, V).unsqueeze(0)
                    g.top_preds = torch.cat([g.top_preds[:, keep], word], 0)
                    g.alphas = torch.cat([g.alphas[:, keep], alpha.unsqueeze(0)[:, keep]], 0)
                    g.h, g.c = g.h[:, keep], g.c[:, keep]
                    g.annots = g.annots[keep]
                kept = g.top_preds[step + 1].tolist()
                if trace is not None:
                    trace.append((idx, step, gi, kept))
                for v in kept:
                    count[v] += 1.0

                def rescore(s, step):
                    if rescore_method == "LN":
                        return s / step
                    if rescore_method == "WR":
                        return s + rescore_reward * step
                    if rescore_method == "BAR":
                        return s + rescore_reward * (-torch.mean(g.top_scores))
                    return s

                def finish(i):
                    g.caps.append(g.top_preds[:, i][1:-1].tolist())
                    g.fin_alphas.append(g.alphas[:, i][1:-1].clone())
                    g.scores.append(float(rescore(g.top_scores[i], step)))
                    g.ppl.append(float(torch.exp(-g.top_scores[i] / step)))

                complete = g.top_preds[step + 1] == END
                if bool(complete.any()):
                    for i in torch.nonzero(complete).flatten().tolist():
                        finish(i)
                    inc = ~complete
                    g.top_preds, g.alphas, g.top_scores = g.top_preds[:, inc], g.alphas[:, inc], g.top_scores[inc]
                    g.h, g.c, g.annots = g.h[:, inc], g.c[:, inc], g.annots[inc]
                    g.k = int(inc.sum())
                    if g.k == 0:
                        g.done = True
                        continue
                if step >= max_gen_length:
                    for i in range(g.top_preds.shape[1]):
                        finish(i)
                    g.done = True
            step += 1
        fin_caps = [c for g in groups for c in g.caps]; fin_alphas = [a for g in groups for a in g.fin_alphas]
        fin_scores = [s for g in groups for s in g.scores]; fin_ppl = [p for g in groups for p in g.ppl]
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
