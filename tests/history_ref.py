"""CPU reference of the history rules of the caption search ("History rules"): repetition penalty, minimum length,
no-repeat n-gram.  Plain Python over lists plus the oracle's own decoder pieces; no GPU, and nothing shared with the kernels or with
``SATDecoder.beam_decode``'s torch formulation.

A live row of step s (0-based) has the history w_1 .. w_s, the words fed at steps 1..s without <START>.  In this order:
1. penalty theta on the raw logits of every distinct history word, once: x > 0 ? x / theta : x * theta; then log-softmax(x / T) + parent
2. the START / PAD (/ END / UNK at step 0) masks
3. s < min_length: score[END] = -inf
4. s >= n - 1: every p in 0 .. s - n with hist[p : p + n - 1] == the last n - 1 words blocks hist[p + n - 1]"""
import torch
import torch.nn.functional as F

from oracle import sat_oracle as O


def blocked_words(hist, n):
    """the words that would say an n-gram of ``hist`` a second time (a set); n = 1: every word already used"""
    hist, s = list(hist), len(hist)
    if n < 1 or s < n - 1:
        return set()
    tail = hist[s - (n - 1):] if n > 1 else []
    return {hist[p + n - 1] for p in range(0, s - n + 1) if hist[p:p + n - 1] == tail}


def penalise(logits, hist, theta):
    """a copy of the 1-D fp32 ``logits`` with the penalty on every distinct word of ``hist``"""
    x = logits.clone()
    t = torch.tensor(float(theta), dtype=logits.dtype)
    for v in sorted(set(int(w) for w in hist)):
        x[v] = x[v] / t if float(x[v]) > 0 else x[v] * t
    return x


def _boundary_gap(flat, k):
    """|k-th - (k+1)-th| of the finite entries, or None when no (k+1)-th exists"""
    s = torch.sort(flat[torch.isfinite(flat)], descending=True).values
    return float(s[k - 1] - s[k]) if len(s) > k else None


def beam_search(sd, hp, ann_img, beamk=3, max_gen_length=32, temperature=1.0, rescore_method=None, rescore_reward=0.5, return_all=False,
                no_repeat_ngram=0, min_length=0, repetition_penalty=1.0, margins=None):
    """``oracle.sat_oracle.beam_search`` ("beam" sampling, no noise) under the history rules; with every rule off the very same
    operations.  ``margins``: a dict that receives "boundary" (at every selection the gap between the last kept and the first dropped
    finite score) and "final" (per image, the gaps between neighbouring final scores of its hypotheses)."""
    stoi = hp.vocab_stoi
    START, PAD, END, UNK = int(stoi["<START>"]), int(stoi["<PAD>"]), int(stoi["<END>"]), int(stoi["<UNK>"])
    V, layers, n = hp.vocab_size, hp.decoder_layers, hp.decoder_dim
    temps = temperature if isinstance(temperature, list) else [temperature]
    ngram, theta = int(no_repeat_ngram), float(repetition_penalty)
    if margins is not None:
        margins.setdefault("boundary", []); margins.setdefault("final", [])
    captions, cap_scores, cap_alphas, cap_ppl = [], [], [], []
    _, _, Hh, Ww = ann_img.shape
    for idx in range(ann_img.shape[0]):
        k = beamk
        annots = ann_img[idx].expand(k, *ann_img[idx].shape)
        h, c = O.init_state(sd, annots, layers, n)
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
            y = O.embed(sd, top_preds[step])
            z, alpha = O.soft_attention(sd, annots, h[-1])
            x = torch.cat([y, O.beta_gate(sd, h[-1]) * z], dim=1).unsqueeze(0)
            h, c = O.lstm_step(sd, x, h, c, layers)
            logits = O.deep_output(sd, y, h[-1], z, hp.deep_output)
            hists = [top_preds[1:step + 1, i].tolist() for i in range(k)]
            if theta != 1.0 and step > 0:
                logits = torch.stack([penalise(logits[i], hists[i], theta) for i in range(k)])
            scores = F.log_softmax(logits / T, dim=1)
            scores[:, [START, PAD]] = float("-inf")
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
                h, c = h[:, keep], c[:, keep]
                annots = annots[keep]
            complete = top_preds[step + 1] == END
            if bool(complete.any()):
                for i in torch.nonzero(complete).flatten().tolist():
                    fin_caps.append(top_preds[:, i][1:-1].tolist())
                    fin_alphas.append(alphas[:, i][1:-1].clone())
                    fin_scores.append(float(rescore(top_scores[i], step)))
                    fin_ppl.append(float(torch.exp(-top_scores[i] / step)))
                inc = ~complete
                top_preds, alphas, top_scores = top_preds[:, inc], alphas[:, inc], top_scores[inc]
                h, c, annots = h[:, inc], c[:, inc], annots[inc]
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


def repeats_ngram(caption, n, free_from=0):
    """does ``caption`` say an n-gram twice?  n-grams lying wholly inside the first ``free_from`` (forced) words are not counted against
    one another, but an n-gram that ends in the free part must not repeat any earlier one"""
    grams = [tuple(caption[p:p + n]) for p in range(len(caption) - n + 1)]
    for q in range(len(grams)):
        if q + n <= free_from:
            continue
        if grams[q] in grams[:q]:
            return True
    return False
