"""Validation metrics of ``SAT.score_captions`` (reference model.py:646-682) without nltk.

The reference calls ``nltk.translate.bleu_score.corpus_bleu`` and ``nltk.translate.gleu_score.corpus_gleu``
(nltk 3.6.2, requirements.txt:6 -- a third-party dependency that is not installed here).  The two functions below restate
the published algorithms of those nltk functions over token-id lists:

* BLEU (Papineni et al. 2002) as nltk computes it at corpus level: clipped n-gram counts and hypothesis n-gram totals summed
  over the corpus per order, brevity penalty from the summed closest reference lengths, geometric mean over the weights
  with nltk's default ``SmoothingFunction().method0`` (an order without any match contributes ``log(sys.float_info.min)``),
  0 when there is no unigram match.
* GLEU (Wu et al. 2016) at corpus level: per hypothesis the reference with the best tp / max(tp+fp, tp+fn) over all 1..4-grams,
  matches and totals summed over the corpus.

Parity: unpinned against nltk itself (absent).  Pinned against the reference's own independent BLEU, ``token_bleu``
(dev/dev_corpus_metrics.py:19-55, imported to generate tests/golden/g10_metrics.npz) wherever the two definitions coincide
(every weighted order has a match), and against hand-computed cases."""
import math
import sys
from collections import Counter
from fractions import Fraction


def _ngrams(seq, n):
    return [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]


def modified_precision(references, hypothesis, n):
    """clipped matches / hypothesis n-grams of one segment (nltk.translate.bleu_score.modified_precision)"""
    counts = Counter(_ngrams(hypothesis, n)) if len(hypothesis) >= n else Counter()
    max_counts = {}
    for ref in references:
        ref_counts = Counter(_ngrams(ref, n)) if len(ref) >= n else Counter()
        for ng in counts:
            max_counts[ng] = max(max_counts.get(ng, 0), ref_counts[ng])
    clipped = sum(min(c, max_counts.get(ng, 0)) for ng, c in counts.items())
    return clipped, max(1, sum(counts.values()))


def closest_ref_length(references, hyp_len):
    return min((len(r) for r in references), key=lambda rl: (abs(rl - hyp_len), rl))


def brevity_penalty(closest_ref_len, hyp_len):
    if hyp_len > closest_ref_len:
        return 1.0
    if hyp_len == 0:
        return 0.0
    return math.exp(1 - closest_ref_len / hyp_len)


def corpus_bleu(list_of_references, hypotheses, weights=(0.25, 0.25, 0.25, 0.25)):
    assert len(list_of_references) == len(hypotheses), "one reference set per hypothesis"
    num, den = Counter(), Counter()
    hyp_lengths = ref_lengths = 0
    for references, hypothesis in zip(list_of_references, hypotheses):
        for i in range(1, len(weights) + 1):
            c, t = modified_precision(references, hypothesis, i)
            num[i] += c; den[i] += t
        hyp_lengths += len(hypothesis)
        ref_lengths += closest_ref_length(references, len(hypothesis))
    bp = brevity_penalty(ref_lengths, hyp_lengths)
    if num[1] == 0:
        return 0
    total = 0.0
    terms = []
    for i, w in enumerate(weights, start=1):
        p = Fraction(num[i], den[i]) if num[i] != 0 else None          # method0: no match at this order -> the smallest float
        terms.append(w * math.log(p if p is not None else sys.float_info.min))
    total = math.fsum(terms)
    return bp * math.exp(total)


def corpus_gleu(list_of_references, hypotheses, min_len=1, max_len=4):
    assert len(list_of_references) == len(hypotheses), "one reference set per hypothesis"

    def everygrams(seq):
        return Counter(ng for n in range(min_len, max_len + 1) for ng in _ngrams(seq, n))

    n_match = n_all = 0
    for references, hypothesis in zip(list_of_references, hypotheses):
        hyp = everygrams(hypothesis)
        tpfp = sum(hyp.values())
        best = None
        for ref in references:
            rg = everygrams(ref)
            tpfn = sum(rg.values())
            tp = sum((rg & hyp).values())
            total = max(tpfp, tpfn)
            if total > 0 and (best is None or tp / total > best[0] / best[1]):
                best = (tp, total)
        if best is not None:
            n_match += best[0]; n_all += best[1]
    return 0.0 if n_all == 0 else n_match / n_all


def bleu_from_stats(clipped, total, hyp_len, ref_len, weights=(0.25, 0.25, 0.25, 0.25)):
    """The tail of ``corpus_bleu`` on statistics already summed over the corpus: ``clipped[i]`` / ``total[i]`` the clipped matches and the
    per-segment ``max(1, .)`` hypothesis n-gram totals of order i + 1, ``hyp_len`` / ``ref_len`` the summed hypothesis and closest reference
    lengths (integers)."""
    bp = brevity_penalty(int(ref_len), int(hyp_len))
    if int(clipped[0]) == 0:
        return 0
    terms = []
    for i, w in enumerate(weights):
        p = Fraction(int(clipped[i]), int(total[i])) if int(clipped[i]) != 0 else None          # method0, as in corpus_bleu
        terms.append(w * math.log(p if p is not None else sys.float_info.min))
    return bp * math.exp(math.fsum(terms))


def gleu_from_stats(tp, total):
    """The tail of ``corpus_gleu``: matches and totals of each segment's best reference, summed over the corpus."""
    return 0.0 if int(total) == 0 else int(tp) / int(total)


# ----------------------------------------------------------------------------- consensus metrics: CIDEr-D and ROUGE-L
# The two COCO caption metrics that need nothing but tokens, restated from the published algorithms (Vedantam et al. 2015, the
# "CIDEr-D" of the COCO evaluation server with sigma = 6; Lin 2004, ROUGE-L as the COCO scorer takes it, beta = 1.2) over token-id
# lists.  They are the specification of sat_ngram_table_add / sat_caption_consensus (csrc/caption_consensus.hip): plain dictionaries,
# fp64.  A reference here is the token list without START and END, as everywhere in this file.

def document_frequency(list_of_references):
    """``{n-gram tuple: number of images whose references contain it}`` over all 1..4-grams.  An image counts once, however often and
    in however many of its references the n-gram occurs."""
    df = Counter()
    for references in list_of_references:
        seen = set()
        for ref in references:
            for n in range(1, 5):
                seen.update(_ngrams(ref, n))
        df.update(seen)
    return dict(df)


def _cider_vector(seq, df, log_n):
    """per order n = 1..4: ``{n-gram: tf * (log N - log max(1, df))}`` in first-occurrence order, its norm, and the scorer's length
    (the number of bigram positions)"""
    vec, norm = [], []
    for n in range(1, 5):
        tf = Counter(_ngrams(seq, n))
        w = {g: float(c) * (log_n - math.log(max(1.0, float(df.get(g, 0))))) for g, c in tf.items()}
        vec.append(w)
        norm.append(math.sqrt(sum(x * x for x in w.values())))
    return vec, norm, max(len(seq) - 1, 0)


def cider_d(list_of_references, hypotheses, df=None, n_images=None, sigma=6.0):
    """CIDEr-D of every image as the COCO scorer computes it (a list; the corpus score is its mean).  ``df`` / ``n_images``: the
    document frequencies and the image count of the corpus the weights come from; by default those of ``list_of_references`` itself."""
    assert len(list_of_references) == len(hypotheses), "one reference set per hypothesis"
    if df is None:
        df = document_frequency(list_of_references)
        if n_images is None:
            n_images = len(list_of_references)
    if n_images is None or int(n_images) < 1:
        raise ValueError("cider_d: n_images >= 1 goes with an explicit df")
    log_n = math.log(float(int(n_images)))
    scores = []
    for references, hypothesis in zip(list_of_references, hypotheses):
        vec_h, norm_h, len_h = _cider_vector(hypothesis, df, log_n)
        total = [0.0] * 4
        for ref in references:
            vec_r, norm_r, len_r = _cider_vector(ref, df, log_n)
            delta = float(len_h - len_r)
            for n in range(4):
                val = 0.0
                for g, wh in vec_h[n].items():
                    wr = vec_r[n].get(g, 0.0)
                    val += min(wh, wr) * wr
                if norm_h[n] != 0 and norm_r[n] != 0:
                    val /= norm_h[n] * norm_r[n]
                total[n] += val * math.exp(-(delta * delta) / (2.0 * sigma * sigma))
        scores.append(10.0 * ((((total[0] + total[1]) + total[2]) + total[3]) / 4.0 / len(references)) if references else 0.0)
    return scores


def lcs_length(a, b):
    """length of the longest common subsequence"""
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0
        for j, y in enumerate(b):
            diag, row[j + 1] = row[j + 1], (diag + 1 if x == y else max(row[j + 1], row[j]))
    return row[len(b)]


def rouge_l(references, hypothesis, beta=1.2):
    """ROUGE-L of one image in the COCO scorer's form: the best LCS precision and the best LCS recall over the references (each its
    own maximum), F with beta = 1.2.  An empty hypothesis scores 0; an empty reference contributes 0."""
    if len(hypothesis) == 0:
        return 0.0
    prec = rec = 0.0
    for ref in references:
        lcs = lcs_length(ref, hypothesis)
        prec = max(prec, lcs / float(len(hypothesis)))
        rec = max(rec, lcs / float(len(ref)) if len(ref) else 0.0)
    if prec != 0 and rec != 0:
        return ((1 + beta ** 2) * prec * rec) / float(rec + beta ** 2 * prec)
    return 0.0


# ----------------------------------------------------------------------------- consensus (minimum-Bayes-risk) reranking
# The captioning literature's way to choose among the finished hypotheses of a beam (Devlin et al. 2015; MBR decoding in MT): keep the
# one that agrees most with the others under the metric the captions are evaluated on.  The specification of sat_caption_mbr
# (csrc/caption_mbr.hip): the two functions above with "the references" of hypothesis i being one other hypothesis j at a time.

def consensus_utilities(hyps, logps, df, n_images, reward=(1.0, 0.0), alpha=0.0, sigma=6.0):
    """``U_i`` of every hypothesis of ONE image (token lists without START / END, in append order; ``logps`` their raw scores):

        gain(i|j) = wc * cider_d([[h_j]], [h_i])[0] + wr * rouge_l([h_j], h_i)      a weight of 0 skips its term
        q_j       = exp(alpha * (s_j - max_k s_k))                                 alpha = 0: every q_j = 1 (uniform consensus)
        U_i       = (sum_{j != i} q_j * gain(i|j)) / (sum_{j != i} q_j)            j ascending; 0 when the denominator is 0 (F = 1)

    with the document frequencies ``df`` of a corpus of ``n_images`` images.  The winner is the first maximum:
    ``u.index(max(u))``."""
    wc, wr, alpha = float(reward[0]), float(reward[1]), float(alpha)
    for x in (wc, wr, alpha):
        if not (x >= 0.0 and x < math.inf):
            raise ValueError("consensus_utilities: weights and alpha are finite numbers >= 0 (reward=%r alpha=%r)" % (reward, alpha))
    if wc == 0.0 and wr == 0.0:
        raise ValueError("consensus_utilities: both weights are 0 (nothing to agree on)")
    F = len(hyps)
    if alpha != 0.0:
        assert len(logps) == F, "one raw score per hypothesis"
        top = max(float(s) for s in logps) if F else 0.0
        q = [math.exp(alpha * (float(s) - top)) for s in logps]
    else:
        q = [1.0] * F
    out = []
    for i in range(F):
        num = den = 0.0
        for j in range(F):
            if j == i:
                continue
            gain = 0.0
            if wc != 0.0:
                gain = gain + wc * cider_d([[hyps[j]]], [hyps[i]], df=df, n_images=n_images, sigma=sigma)[0]
            if wr != 0.0:
                gain = gain + wr * rouge_l([hyps[j]], hyps[i])
            num += q[j] * gain
            den += q[j]
        out.append(num / den if den != 0.0 else 0.0)
    return out


# ----------------------------------------------------------------------------- chrF: character n-gram F-score
# chrF (Popovic 2015) as nltk's ``chrf_score.py`` computes it (``sentence_chrf`` / ``corpus_chrf`` with ``min_len=1, max_len=6,
# beta=3.0, ignore_whitespace=True``): restated over lists of word strings, nltk being absent here.  It is the specification of
# sat_caption_chrf (csrc/caption_chrf.hip): plain counters, fp64.  The one metric of this file that looks inside words.
CHRF_MAX_ORDER = 6
CHRF_EPSILON = 1e-16          # the F-score of an order that is undefined (no n-gram on one side) or has no match


def chrf_text(words):
    """the Unicode code points (a list of ints) of the words concatenated, every whitespace code point dropped: tokens do not separate
    n-grams ("a man" gives a, m, a, n and the bigram "am" exists)"""
    return [ord(c) for w in words for c in str(w) if not c.isspace()]


def chrf_stats(reference, hypothesis):
    """``(tp, Lh, Lr)``: per order n = 1..6 the matches ``sum over distinct n-grams g of min(count_h(g), count_r(g))``, and the
    character counts of hypothesis and reference"""
    hyp, ref = chrf_text(hypothesis), chrf_text(reference)
    tp = []
    for n in range(1, CHRF_MAX_ORDER + 1):
        ch, cr = Counter(_ngrams(hyp, n)), Counter(_ngrams(ref, n))
        tp.append(sum(min(c, cr[g]) for g, c in ch.items()))
    return tp, len(hyp), len(ref)


def chrf_from_stats(tp, hyp_chars, ref_chars, beta=3.0):
    """the sentence score from the integers of ``chrf_stats``: the mean over all six orders of F_n, summed in ascending n"""
    beta2 = float(beta) * float(beta)
    total = 0.0
    for n in range(1, CHRF_MAX_ORDER + 1):
        nh, nr, t = max(int(hyp_chars) - n + 1, 0), max(int(ref_chars) - n + 1, 0), int(tp[n - 1])
        if nh == 0 or nr == 0 or t == 0:
            f = CHRF_EPSILON
        else:
            p, q = t / nh, t / nr
            f = ((1.0 + beta2) * (p * q)) / (beta2 * p + q)
        total += f
    return total / CHRF_MAX_ORDER


def chrf_sentence(reference, hypothesis, beta=3.0):
    """chrF of one hypothesis against one reference (lists of word strings)"""
    return chrf_from_stats(*chrf_stats(reference, hypothesis), beta=beta)


def chrf(references, hypothesis, beta=3.0):
    """chrF of one image: the maximum over its references"""
    return max(chrf_sentence(ref, hypothesis, beta) for ref in references)


def corpus_chrf(list_of_references, hypotheses, beta=3.0):
    """the mean of the image scores"""
    assert len(list_of_references) == len(hypotheses), "one reference set per hypothesis"
    scores = [chrf(references, hypothesis, beta) for references, hypothesis in zip(list_of_references, hypotheses)]
    return sum(scores) / len(scores)


def distinct_n(captions, n):
    """distinct-n of a list of captions (lists of tokens or words): the number of different n-grams over the number of n-grams, pooled
    over the list (Li et al. 2016).  1.0: no n-gram occurs twice; a list of k copies of one caption without inner repeats gives 1 / k.
    0.0 when no caption has n tokens.  What a diverse beam buys over a plain one ("Diverse beam search")."""
    n = int(n)
    if n < 1:
        raise ValueError("distinct_n: n=%d is not positive" % n)
    grams = [g for c in captions for g in _ngrams(list(c), n)]
    return len(set(grams)) / len(grams) if grams else 0.0


# ----------------------------------------------------------------------------- diversity of a beam: distinct-n, mBLEU, unique captions
# What the searches that return different captions are built to change, as integers up to one final division: distinct-n (Li et al.
# 2016, the "Div-n" of the captioning papers), mBLEU / self-BLEU (every caption scored with the rest of its set as references:
# Vijayakumar et al. 2018, Wang & Chan 2019) and the share of unique captions.  The specification of sat_caption_diversity
# (csrc/caption_diversity.hip).  A hypothesis is the token list without START and END, as everywhere in this file.
DIVERSITY_STATS = 20
DIVERSITY_KEYS = ("distinct1", "distinct2", "distinct3", "distinct4", "mbleu1", "mbleu2", "mbleu3", "mbleu4", "unique", "hypotheses")
#: the weights mBLEU-n is taken with: evaluation.BLEU_WEIGHTS (the reference's, model.py:651-654, bleu3 as written there), restated here
#: because evaluation.py imports this file; tests/test_diversity.py holds the two together
MBLEU_WEIGHTS = {"mbleu1": (1, 0, 0, 0), "mbleu2": (0.5, 0.5, 0, 0), "mbleu3": (0.33, 0.33, 0.33, 0), "mbleu4": (0.25, 0.25, 0.25, 0.25)}


def diversity_per_hypothesis(hyps):
    """per hypothesis of ONE image the 10 BLEU columns of sat_caption_stats with all the OTHER hypotheses as its references (duplicates
    and empty ones stay among them): clipped matches n = 1..4, ``max(1, len - n + 1)`` n = 1..4, the length, the closest other length
    (a tie goes to the shorter).  All 0 for an image with fewer than 2 hypotheses: there is nothing to compare with."""
    hyps = [list(h) for h in hyps]
    if len(hyps) < 2:
        return [[0] * 10 for _ in hyps]
    rows = []
    for i, h in enumerate(hyps):
        others = hyps[:i] + hyps[i + 1:]
        pairs = [modified_precision(others, h, n) for n in range(1, 5)]
        rows.append([p[0] for p in pairs] + [p[1] for p in pairs] + [len(h), closest_ref_length(others, len(h))])
    return rows


def diversity_stats(hyps):
    """the 20 integers of ONE image's hypotheses (the columns of sat_caption_diversity, include/sat_hip.h): ``[0..3]`` distinct n-grams
    pooled over the hypotheses, ``[4..7]`` n-gram positions pooled (``[n-1] / [3+n]`` is ``distinct_n(hyps, n)``), ``[8]`` hypotheses,
    ``[9]`` distinct hypotheses, ``[10..19]`` the columns of ``diversity_per_hypothesis`` summed over the hypotheses."""
    hyps = [list(h) for h in hyps]
    out = [len(set(g for h in hyps for g in _ngrams(h, n))) for n in range(1, 5)]
    out += [sum(max(len(h) - n + 1, 0) for h in hyps) for n in range(1, 5)]
    out += [len(hyps), len(set(tuple(h) for h in hyps))]
    rows = diversity_per_hypothesis(hyps)
    return out + [sum(r[c] for r in rows) for c in range(10)]


def diversity_from_stats(sums, vocab_used=None):
    """the metric dict from the columns of ``diversity_stats`` summed over images: distinct1..4 (0.0 without a position), mbleu1..4
    (``bleu_from_stats`` of the summed self-BLEU columns: the corpus BLEU of every hypothesis against the others of its image), unique
    (distinct hypotheses / hypotheses, 0.0 without one), hypotheses; ``vocabulary`` (the number of different words used) when
    ``vocab_used`` is given."""
    s = [int(x) for x in sums]
    if len(s) != DIVERSITY_STATS:
        raise ValueError("diversity_from_stats: %d numbers (%d)" % (len(s), DIVERSITY_STATS))
    out = {"distinct%d" % n: (s[n - 1] / s[3 + n] if s[3 + n] else 0.0) for n in range(1, 5)}
    for k, w in MBLEU_WEIGHTS.items():
        out[k] = bleu_from_stats(s[10:14], s[14:18], s[18], s[19], w)          # no match at all (all-zero sums included): 0
    out["unique"] = s[9] / s[8] if s[8] else 0.0
    out["hypotheses"] = s[8]
    if vocab_used is not None:
        out["vocabulary"] = int(vocab_used)
    return out
