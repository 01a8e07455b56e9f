"""Host restatement of the per-image statistics of ``sat_caption_stats`` (include/sat_hip.h), written from metrics.py's helpers:
what ``corpus_bleu`` and ``corpus_gleu`` sum per segment, and the corpora the evaluation tests share (CPU and GPU)."""
import os
from collections import Counter

import numpy as np

WEIGHTS = [(1, 0, 0, 0), (0.5, 0.5, 0, 0), (0.33, 0.33, 0.33, 0), (0.25, 0.25, 0.25, 0.25)]


def caption_stats(references, hypothesis):
    """[clipped1..4, total1..4, hyp_len, closest_ref_len, gleu_tp, gleu_total] of one segment"""
    from sat_amd import metrics
    clipped, total = zip(*[metrics.modified_precision(references, hypothesis, n) for n in range(1, 5)])

    def everygrams(seq):
        return Counter(ng for n in range(1, 5) for ng in metrics._ngrams(seq, n))

    hyp = everygrams(hypothesis)
    tpfp = sum(hyp.values())
    best = (0, 0)
    for ref in references:
        rg = everygrams(ref)
        tp, tot = sum((rg & hyp).values()), max(tpfp, sum(rg.values()))
        if tot > 0 and (best[1] == 0 or tp * best[1] > best[0] * tot):          # the same order as tp / tot > best_tp / best_tot, in integers
            best = (tp, tot)
    return list(clipped) + list(total) + [len(hypothesis), metrics.closest_ref_length(references, len(hypothesis)), best[0], best[1]]


def corpus_stats(list_of_references, hypotheses):
    return [caption_stats(r, h) for r, h in zip(list_of_references, hypotheses)]


def random_corpora():
    """seeded corpora: small vocabularies (6..40: n-grams repeat, clipping bites), R 1..5, lengths 0..12"""
    out = {}
    for seed, (nseg, vocab, R) in enumerate([(16, 6, 1), (24, 6, 3), (20, 9, 5), (32, 12, 2), (16, 25, 4), (40, 40, 5), (12, 7, 5), (8, 6, 2)]):
        rs = np.random.RandomState(1000 + seed)
        refs = [[rs.randint(4, 4 + vocab, size=rs.randint(0, 13)).tolist() for _ in range(R)] for _ in range(nseg)]
        caps = [rs.randint(4, 4 + vocab, size=rs.randint(0, 13)).tolist() for _ in range(nseg)]
        out["rand%d_v%d_r%d" % (seed, vocab, R)] = (refs, caps)
    return out


def g10_corpora(golden_dir):
    g = np.load(os.path.join(golden_dir, "g10_metrics.npz"), allow_pickle=False)
    out = {}
    for name in g["names"].tolist():
        refs, caps = [], []
        for i in range(int(g[name + "_nseg"])):
            caps.append(g["%s_cap%d" % (name, i)].tolist())
            refs.append([g["%s_ref%d_%d" % (name, i, j)].tolist() for j in range(int(g["%s_nref%d" % (name, i)]))])
        out["g10_" + name] = (refs, caps)
    return out


def edge_corpora():
    """(references, hypotheses) that isolate one rule each; every segment of a corpus has the same number of references"""
    rs = np.random.RandomState(77)
    lim = ([[rs.randint(4, 9, size=n).tolist() for n in (127, 126, 1, 0, 64, 127, 3, 90, 127, 2, 127, 50, 127, 10, 127, 99)] for _ in range(3)],
           [rs.randint(4, 9, size=n).tolist() for n in (128, 127, 0)])
    return {
        "hyp_shorter_than_n": ([[[5, 6, 7, 8], [5, 6]], [[9, 9, 9, 9], [4]]], [[5, 6], [9]]),
        "hyp_empty": ([[[5, 6, 7], [8, 9]], [[], [4, 5]], [[], []]], [[], [], []]),
        "repeat_once_and_twice": ([[[5, 6, 9, 8], [5, 6, 7, 5, 6]], [[5, 6, 7, 5, 6], [5, 6, 9, 8]]], [[5, 6, 5, 6, 5, 6], [5, 6, 5, 6, 5, 6]]),
        "two_refs_equally_close": ([[[4, 5, 6, 7, 8, 9], [4, 5, 6, 7]], [[4, 5, 6, 7], [4, 5, 6, 7, 8, 9]]], [[4, 5, 6, 7, 8], [9, 8, 7, 6, 5]]),
        # hypothesis [5, 6]: tp + fp = 3; [5, 11] gives 1 / 3, [6, 12, 5] gives 2 / 6: equal ratios, the first one met stays
        "equal_gleu_ratio": ([[[5, 11], [6, 12, 5]], [[6, 12, 5], [5, 11]]], [[5, 6], [5, 6]]),
        "at_the_limits": lim,            # cap_width 128, T 128, R 16
    }


def pack(references, hypotheses, start=1, pad=0, width=None, T=None):
    """the corpus as the tensors the kernels take: tokens (B, W), lengths (B), refs (B, R, T) = [START, tokens..., PAD...] with
    ref_lengths = len + 1 so that c[1:l] is the reference.  Segments with fewer references than the widest repeat their LAST one, which
    changes no statistic (maxima, the closest length and the strictly-better rule ignore a duplicate)."""
    B, R = len(hypotheses), max(len(r) for r in references)
    W = width or max(1, max(len(h) for h in hypotheses))
    T = T or max(len(x) for r in references for x in r) + 2
    tokens, lengths = np.full((B, W), pad, np.int32), np.zeros(B, np.int32)
    refs, ref_lengths = np.full((B, R, T), pad, np.int32), np.zeros((B, R), np.int32)
    for b, (rl, h) in enumerate(zip(references, hypotheses)):
        tokens[b, :len(h)] = h; lengths[b] = len(h)
        for r in range(R):
            x = rl[min(r, len(rl) - 1)]
            refs[b, r, 0] = start; refs[b, r, 1:1 + len(x)] = x; ref_lengths[b, r] = len(x) + 1
    return tokens, lengths, refs, ref_lengths
