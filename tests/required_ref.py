"""CPU reference of the required words of the batched caption search ("Required words"; include/sat_hip.h,
sat_beam_search_required): ``history_ref.beam_search``'s step with the selection restated in numpy float32.  No GPU, nothing shared with
the kernels.

Image b requires the words q_0 .. q_{C-1}.  With s[j, v] the scores of every search, per step and image:
  met(j)      the c whose q_c row j has said
  END held    s'[j, END] = -inf while met(j) is not everything
  candidates  the union by flat index j * V + v of  A: the k picks of the plain rule over s' (value descending, ties to the lower flat
              index), those at -inf dropped;  R: (j, q_c) for c not in met(j), where s' > -inf;  M: every row's best word (the lowest v on
              ties), where s' > -inf
  bank        |met(j) U {c : q_c == v}|; at the last step |met(j)|: the word picked there is <END> or is dropped by the cut, so it is not
              part of the caption (counting it lets a hypothesis that completes with the dropped word push a complete one out)
  allocation  a pointer p starts at C; pick t walks the banks p, p - 1, .., 0, C, .., p + 1 to the first that holds an untaken candidate,
              takes its best (value descending, ties to the lower flat index) and sets p = (bank - 1) mod (C + 1); nothing left: -inf / 0
The pick carries s', never anything else.  An image without words takes the plain rule's picks.  After the search the finished list of an
image keeps, in order, the hypotheses that contain the most required words; that count is req_met."""
import numpy as np
import torch
import torch.nn.functional as F

import history_ref as HR
from oracle import sat_oracle as O

NEG = np.float32(-np.inf)


def plain_picks(x, k):
    """sat_topk's rule on the flat float32 ``x``: value descending, ties to the lower index, -inf last in index order"""
    return np.argsort(-x, kind="stable")[:k]


def select_image(x, k, hists, words, V, end_id, gaps=None, last=False):
    """One image: ``x`` (rows, V) float32, the rows' histories (lists of ids), its required ``words``.  Returns (values, indices) of the
    k picks.  ``gaps`` (a list) receives what the picks rest on: per bank the gap between its last kept and its first dropped candidate;
    where the last pick of A was taken, the gap at the boundary of A (its neighbour would have been the candidate); where a word that only
    M brought in was taken, the gap to the row's second best."""
    rows = x.shape[0]
    words = [int(w) for w in words if 0 <= int(w) < V]
    C = len(words)
    if C == 0:
        pick = plain_picks(x.reshape(-1), k)
        return x.reshape(-1)[pick].astype(np.float32), pick.astype(np.int32)
    met = [{c for c in range(C) if words[c] in hists[j]} for j in range(rows)]
    s = x.astype(np.float32).copy()
    for j in range(rows):
        if len(met[j]) < C and 0 <= end_id < V:
            s[j, end_id] = NEG
    flat = s.reshape(-1)
    A = [int(i) for i in plain_picks(flat, k) if flat[i] > NEG]
    R = [j * V + words[c] for j in range(rows) for c in range(C) if c not in met[j] and s[j, words[c]] > NEG]
    M = [j * V + int(np.argmax(s[j])) for j in range(rows) if s[j].max() > NEG]          # argmax: the first of equal maxima
    cand = sorted(set(A) | set(R) | set(M))
    def bank(i):
        j, v = divmod(i, V)
        return len(met[j]) if last else len(met[j] | {c for c in range(C) if words[c] == v})

    banks = [[] for _ in range(C + 1)]
    for i in cand:
        banks[bank(i)].append(i)
    for bk in banks:
        bk.sort(key=lambda i: (-float(flat[i]), i))                                        # value descending, ties to the lower flat index
    taken = [0] * (C + 1)
    values = np.full(k, NEG, np.float32); indices = np.zeros(k, np.int32)
    p = C
    for t in range(k):
        for u in range(C + 1):
            bk = (p - u) % (C + 1)
            if taken[bk] < len(banks[bk]):
                i = banks[bk][taken[bk]]
                taken[bk] += 1
                values[t], indices[t] = flat[i], i
                p = (bk - 1) % (C + 1)
                break
    if gaps is not None:
        picked = {int(i) for i, v in zip(indices, values) if v > NEG}
        fin = np.sort(flat[np.isfinite(flat)])[::-1]
        if len(fin) > k and len(A) == k and A[-1] in picked:
            gaps.append(float(fin[k - 1] - fin[k]))
        for i in (set(M) - set(A) - set(R)) & picked:
            row = np.sort(s[i // V][np.isfinite(s[i // V])])[::-1]
            if len(row) > 1:
                gaps.append(float(row[0] - row[1]))
        for bk in range(C + 1):
            if 0 < taken[bk] < len(banks[bk]):
                gaps.append(float(flat[banks[bk][taken[bk] - 1]] - flat[banks[bk][taken[bk]]]))
    return values, indices


def select(scores, klive, hist, step, words, n_words, first, end_id):
    """sat_beam_required_select restated: scores (B, K, V) float32, klive (B), hist (B * K, stride) int with ``step`` valid entries per
    row, words (B, C), n_words (B); first & 1: row 0 alone, first & 2: the last step.  Returns (values (B, K) float32, indices (B, K) int32); slots the kernel leaves untouched hold
    NaN / -7."""
    scores = np.asarray(scores, np.float32)
    B, K, V = scores.shape
    hist = np.asarray(hist).reshape(B, K, -1)
    words = np.asarray(words).reshape(B, -1)
    C = words.shape[1]
    values = np.full((B, K), np.nan, np.float32); indices = np.full((B, K), -7, np.int32)
    L = int(np.clip(step, 0, hist.shape[2]))
    for b in range(B):
        k = int(np.clip(klive[b], 0, K))
        if k == 0:
            continue
        rows = 1 if int(first) & 1 else k
        nb = int(np.clip(n_words[b], 0, C)) if C else 0
        hists = [hist[b, j, :L].tolist() for j in range(rows)]
        values[b, :k], indices[b, :k] = select_image(scores[b, :rows], k, hists, words[b, :nb].tolist(), V, int(end_id), last=bool(int(first) & 2))
    return values, indices


def count_required(caption, words):
    """how many of ``words`` the caption (a list of ids) says"""
    said = {int(t) for t in caption}
    return sum(1 for w in words if int(w) in said)


def sequence_logprob(sd, hp, ann_one, words, temperature=1.0, beamk=1, first_row=0):
    """``group_ref.sequence_logprob`` for a hypothesis of a beam of ``beamk`` rows: the sum of log-softmax(logits / T_s)[words[s]],
    teacher-forcing <START>, words[0], ...  The reshape of the initial state depends on the row count, and the search scores
    the first word on row 0 but carries on from the state of the slot the word was kept in, ``first_row``; so the first step runs on
    all ``beamk`` rows as the search does, the rest on that slot's row alone.  beamk = 1 is ``group_ref.sequence_logprob``."""
    temps = temperature if isinstance(temperature, list) else [temperature]
    annots = ann_one.unsqueeze(0).expand(beamk, *ann_one.shape)
    h, c = O.init_state(sd, annots, hp.decoder_layers, hp.decoder_dim)
    fed, total = torch.full((beamk,), int(hp.vocab_stoi["<START>"]), dtype=torch.long), torch.zeros(())
    for s, w in enumerate(words):
        y = O.embed(sd, fed)
        z, _ = O.soft_attention(sd, annots, h[-1])
        x = torch.cat([y, O.beta_gate(sd, h[-1]) * z], dim=1).unsqueeze(0)
        h, c = O.lstm_step(sd, x, h, c, hp.decoder_layers)
        logits = O.deep_output(sd, y, h[-1], z, hp.deep_output)
        total = total + F.log_softmax(logits / temps[s % len(temps)], dim=1)[0, int(w)]
        if s == 0:
            h, c, annots = h[:, first_row:first_row + 1], c[:, first_row:first_row + 1], annots[first_row:first_row + 1]
        fed = torch.tensor([int(w)])
    return float(total)


def beam_search(sd, hp, ann_img, beamk=3, max_gen_length=32, temperature=1.0, rescore_method=None, rescore_reward=0.5, return_all=False,
                no_repeat_ngram=0, min_length=0, repetition_penalty=1.0, banned=(), required=None, margins=None, info=None):
    """``history_ref.beam_search`` with banned ids and required words: ``required`` is None or one list of ids per image.  An image
    without words runs the very operations of ``history_ref.beam_search``.  ``margins`` as there ("boundary": every gap ``select_image``
    reports, or the plain boundary gap).  ``info``: a dict that receives "req_met" (per image) and "ended" (per image, for every finished
    hypothesis before the compaction: did it end by saying <END>, and how many required words it contains) and "said" (per image, for
    every finished hypothesis before the compaction: its words with the closing <END> or cut word, the slot its first word was kept in,
    its raw score)."""
    stoi = hp.vocab_stoi
    START, PAD, END, UNK = int(stoi["<START>"]), int(stoi["<PAD>"]), int(stoi["<END>"]), int(stoi["<UNK>"])
    V, layers, n = hp.vocab_size, hp.decoder_layers, hp.decoder_dim
    temps = temperature if isinstance(temperature, list) else [temperature]
    ngram, theta, banned = int(no_repeat_ngram), float(repetition_penalty), [int(t) for t in banned]
    if margins is not None:
        margins.setdefault("boundary", []); margins.setdefault("final", [])
    if info is not None:
        info.setdefault("req_met", []); info.setdefault("ended", []); info.setdefault("said", [])
    captions, cap_scores, cap_alphas, cap_ppl = [], [], [], []
    _, _, Hh, Ww = ann_img.shape
    for idx in range(ann_img.shape[0]):
        words = [int(w) for w in required[idx]] if required is not None else []
        k = beamk
        annots = ann_img[idx].expand(k, *ann_img[idx].shape)
        h, c = O.init_state(sd, annots, layers, n)
        top_preds = torch.full((1, k), START, dtype=torch.long)
        top_scores = torch.zeros(k)
        alphas = torch.zeros(1, k, Hh, Ww)
        fin_caps, fin_alphas, fin_scores, fin_ppl, fin_by_end, fin_said = [], [], [], [], [], []
        origin = torch.arange(k)

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
            seq = scores[0:1] if step == 0 else scores + top_scores.unsqueeze(1)
            if words:
                gaps = [] if margins is not None else None
                _, pick = select_image(seq.numpy(), k, hists[:seq.shape[0]], words, V, END, gaps, last=step >= max_gen_length)
                if margins is not None:
                    margins["boundary"].append(min(gaps) if gaps else None)
                pred_idx = torch.from_numpy(pick.astype(np.int64))
            else:
                if margins is not None:
                    margins["boundary"].append(HR._boundary_gap(seq.reshape(-1), k))
                _, pred_idx = torch.topk(seq.reshape(-1), k, dim=0)
            if step == 0:
                top_scores = seq.reshape(-1)[pred_idx]
                top_preds = torch.cat([top_preds, pred_idx.unsqueeze(0)], 0)
                alphas = torch.cat([alphas, alpha.unsqueeze(0)], 0)
            else:
                top_scores = seq.reshape(-1)[pred_idx]
                keep = torch.div(pred_idx, V, rounding_mode="floor")
                word = torch.remainder(pred_idx, V).unsqueeze(0)
                top_preds = torch.cat([top_preds[:, keep], word], 0)
                alphas = torch.cat([alphas[:, keep], alpha.unsqueeze(0)[:, keep]], 0)
                h, c = h[:, keep], c[:, keep]
                annots = annots[keep]
                origin = origin[keep]
            complete = top_preds[step + 1] == END
            if bool(complete.any()):
                for i in torch.nonzero(complete).flatten().tolist():
                    fin_caps.append(top_preds[:, i][1:-1].tolist())
                    fin_alphas.append(alphas[:, i][1:-1].clone())
                    fin_scores.append(float(rescore(top_scores[i], step)))
                    fin_ppl.append(float(torch.exp(-top_scores[i] / step)))
                    fin_by_end.append(True)
                    fin_said.append((top_preds[:, i][1:].tolist(), int(origin[i]), float(top_scores[i])))
                inc = ~complete
                origin = origin[inc]
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
                    fin_by_end.append(False)
                    fin_said.append((top_preds[:, i][1:].tolist(), int(origin[i]), float(top_scores[i])))
                break
            step += 1
        # the finished list keeps the hypotheses that contain the most required words, order kept
        counts = [count_required(cap, words) for cap in fin_caps]
        best = max(counts)
        if info is not None:
            info["req_met"].append(best); info["ended"].append(list(zip(fin_by_end, counts))); info["said"].append(fin_said)
        kept = [i for i in range(len(fin_caps)) if counts[i] == best]
        fin_caps = [fin_caps[i] for i in kept]; fin_alphas = [fin_alphas[i] for i in kept]
        fin_scores = [fin_scores[i] for i in kept]; fin_ppl = [fin_ppl[i] for i in kept]
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
