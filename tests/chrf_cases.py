"""Cases shared by test_chrf.py (host) and test_gpu_chrf.py (device): the worked example of chrF, a small vocabulary whose
three-letter alphabet makes character n-grams repeat across word boundaries, a random corpus over it, and the kernel's counting
identity restated in Python."""
import numpy as np

#: the worked example: words, per reference (tp for n = 1..6, Lh, Lr) and the sentence score; fp64 from the definition
HYP = "a man rides a wave".split()
REFS = ["a man riding a wave".split(), "man on a surfboard".split(), "a surfer rides the wave".split()]
STATS = [([12, 10, 8, 6, 4, 2], 14, 15), ([8, 2, 1, 0, 0, 0], 14, 15), ([10, 7, 5, 3, 1, 0], 14, 19)]
SENTENCE = [0.5363571644108024, 0.12638617060152416, 0.2510141246514995]
IMAGE, IMAGE_BETA2 = 0.5363571644108024, 0.540562511877475
CAT = (["a", "cat"], ["cat"], [(3, 3, 4), (2, 2, 3), (1, 1, 2), (0, 0, 1), (0, 0, 0), (0, 0, 0)], 0.3308669551863744)     # ref, hyp, (tp, nh, nr), score
CAFE = ("café 日本".split(), "cafe 日本".split(), 0.28055555555555556)                                 # ref, hyp, score

#: twelve words over a, b, c (and three words outside it); id 11 is absent from the mapping and spells <UNK>
WORDS = ["a", "ab", "ba", "aab", "abc", "cab", "bcabca", "c", "é", "日本", "abab"]
VOCAB_ITOS = dict(enumerate(WORDS))
VOCAB_SIZE = 12


def spell(ids, itos=VOCAB_ITOS):
    """token ids -> word strings, as ``SAT.itos`` spells them"""
    return [str(itos.get(int(i), "<UNK>")) for i in ids]


def example_ids():
    """the worked example as token ids over its own vocabulary: ``(vocab_itos, vocab_size, refs, hyp)``"""
    words = sorted({w for s in REFS + [HYP] for w in s})
    stoi = {w: i for i, w in enumerate(words)}
    return dict(enumerate(words)), len(words), [[stoi[w] for w in r] for r in REFS], [stoi[w] for w in HYP]


def random_corpus(B=37, R=5, T=24, vocab=VOCAB_SIZE, seed=23):
    """``(refs, hyps)`` as token-id lists: hypothesis lengths 0..T - 1 (image b < T has b tokens), references from empty (stored
    length 1: START only) to T - 1 tokens, duplicated references, a hypothesis that repeats a reference's start three times (its
    n-gram counts exceed the reference's) and hypotheses that copy a reference."""
    rs = np.random.RandomState(seed)
    refs, hyps = [], []
    for b in range(B):
        rr = [rs.randint(0, vocab, size=rs.randint(0, T)).tolist() for _ in range(R)]
        if b % 3 == 0:
            rr[3] = list(rr[0])
        if b % 5 == 0:
            rr[1] = []
        if b % 7 == 0:
            rr[2] = rs.randint(0, vocab, size=T - 1).tolist()
        refs.append(rr)
        hyps.append(list(rr[b % R]) if b >= T and b % 4 == 0 else rs.randint(0, vocab, size=b % T).tolist())
    refs[25][0] = [4, 6, 1, 5, 0]
    hyps[25] = (refs[25][0][:3] * T)[:T - 1]
    return refs, hyps


def walk_tp(hyp, ref, orders=6):
    """tp_1..tp_6 the way csrc/caption_chrf.hip counts them, over code-point lists: hypothesis position i contributes 1 to tp_n iff
    the number of EARLIER hypothesis positions with the same n-gram is smaller than the number of reference positions with it.  Both
    counts come from the length of the common run, capped at six, of two windows; sentinels behind the sentences end every run."""
    h, r = list(hyp) + [-2] * 8, list(ref) + [-1] * 8

    def run(a, i, b, j):
        m = 0
        while m < orders and a[i + m] == b[j + m]:
            m += 1
        return m

    tp = [0] * orders
    for i in range(len(hyp)):
        prev, cr = [0] * orders, [0] * orders
        for j in range(i):
            for n in range(run(h, i, h, j)):
                prev[n] += 1
        for j in range(len(ref)):
            for n in range(run(h, i, r, j)):
                cr[n] += 1
        for n in range(orders):
            tp[n] += 1 if prev[n] < cr[n] else 0
    return tp
