"""Cases shared by test_diversity.py (host) and test_gpu_diversity.py (device): beams of hypotheses over a vocabulary of 3 - 5 words, so
that repeats and collisions are the rule, with the planted edge cases of sat_caption_diversity, their packing into the kernel's layout
and the host specification (sat_amd/metrics.py: diversity_stats, diversity_per_hypothesis) of every image, computed once per shape.  No
GPU use.

Image b of ``beams(K, width)``:
    0 .. K     b hypotheses (every count)
    K + 1      identical hypotheses                                  K + 2   hypotheses that are all empty
    K + 3      [1,1,1,1] beside [1] (clipping matters), then lengths 0, 1, 2, 3 (shorter than n for every n) and a full-width one
    K + 4      lengths 3 / 1 / 5 (1 / 0 / 2 below width 5): the others of the first are equally far from it, the tie goes to the shorter
    K + 5      a full beam whose packed hyp_count is K + 3 and whose full-width hypothesis is packed with hyp_len = width + 5 (clamped)
    K + 6      tokens 65534, 65535, 70000 and -5: the specification applies to the tokens clamped into [0, 65534]
    K + 7      a full beam of ordinary captions
Where K or width leave no room (K = 1, width = 1) a planted image keeps the part that fits; ``planted`` says which shapes hold what.
Image 0 is packed with hyp_count = -2 and the first empty hypothesis of image K + 2 with hyp_len = -3 (clamped to 0)."""
import numpy as np

#: (K, width): one hypothesis, width 1, odd middles, a width that is no multiple of the wave, the limits
SHAPES = [(1, 4), (2, 1), (3, 5), (5, 10), (7, 33), (32, 128)]
MAX_IMAGES = 40
BIG_TOKENS = [65534, 65535, 70000, -5]
GARBAGE = 2           # the token of the unused slots: a word of the vocabulary, so that reading it would change the counts

_beams, _expected = {}, {}


def beams(K, width):
    """the images of shape (K, width): per image a list of at most K hypotheses, each a list of at most ``width`` RAW tokens"""
    if (K, width) in _beams:
        return _beams[(K, width)]
    rs = np.random.RandomState(17 + 1000 * K + width)
    vocab = 3 + (K + width) % 3                       # 3, 4 or 5 words
    short = min(width, 9)                             # most hypotheses are caption-sized, so that the host specification stays quick

    def draw(n=None):
        n = rs.randint(0, short + 1) if n is None else n
        return rs.randint(0, vocab, size=n).tolist()

    hyps = [[draw() for _ in range(c)] for c in range(K + 1)]
    dup = draw(min(width, 2))
    hyps.append([list(dup) for _ in range(min(K, 4))])
    hyps.append([[] for _ in range(min(K, 3))])
    hyps.append(([[1, 1, 1, 1][:width], [1], [], draw(1), draw(min(2, width)), draw(min(3, width)), draw(width)] + [draw() for _ in range(K)])[:K])
    tie = (3, 1, 5) if width >= 5 else (1, 0, 2)
    hyps.append(([draw(n) for n in tie] + [draw(tie[1 + i % 2]) for i in range(K)])[:K])
    hyps.append(([draw(width)] + [draw() for _ in range(K)])[:K])
    hyps.append(([BIG_TOKENS[:width], [65535, 65534][:width], [70000], [65534], draw()] + [draw() for _ in range(K)])[:K])
    hyps.append([draw(min(3, width))] + [draw(rs.randint(min(2, width), short + 1)) for _ in range(K - 1)])
    assert len(hyps) == K + 8 <= MAX_IMAGES
    _beams[(K, width)] = hyps
    return hyps


def clamped(hyps):
    """the hypotheses as the n-gram keys see them (caption_ngram.h, key_token): tokens clamped into [0, 65534]"""
    return [[[min(max(int(t), 0), 65534) for t in h] for h in image] for image in hyps]


def pack(hyps, K, width):
    """-> numpy ``(hyp_tokens (B, K, width) int32, hyp_len (B, K) int32, hyp_count (B) int32)``; the unused slots and the tokens behind a
    hypothesis's end carry a word and lengths that must not be read; the out-of-range counts and lengths of the module docstring"""
    B = len(hyps)
    tok = np.full((B, K, width), GARBAGE, np.int32)
    ln, cnt = np.full((B, K), width, np.int32), np.zeros(B, np.int32)
    for b, image in enumerate(hyps):
        cnt[b] = len(image)
        for f, h in enumerate(image):
            tok[b, f, :len(h)] = h
            ln[b, f] = len(h)
    cnt[0] = -2
    ln[K + 2, 0] = -3
    assert len(hyps[K + 5]) == K and len(hyps[K + 5][0]) == width
    cnt[K + 5] = K + 3
    ln[K + 5, 0] = width + 5
    return tok, ln, cnt


def expected(K, width):
    """``(stats, per_hyp)`` of every image of ``beams(K, width)`` from the host specification, as nested lists: (B, 20) and (B, K, 10)
    with the unused slots 0.  Computed once per shape, shared, left unchanged."""
    if (K, width) not in _expected:
        import sat_amd  # noqa: F401
        from sat_amd import metrics
        stats, per_hyp = [], []
        for image in clamped(beams(K, width)):
            stats.append(metrics.diversity_stats(image))
            per_hyp.append(metrics.diversity_per_hypothesis(image) + [[0] * 10 for _ in range(K - len(image))])
        _expected[(K, width)] = (stats, per_hyp)
    return _expected[(K, width)]


def planted(K, width):
    """which of the planted cases shape (K, width) has room for"""
    return dict(identical=K >= 2, all_empty=True, clipping=K >= 2 and width >= 4, short=K >= 6, full_width=True, tie=K >= 3 and width >= 2,
                clamp=True, big_tokens=True)
