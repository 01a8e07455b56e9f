"""Cases shared by test_consensus.py (host) and test_gpu_consensus.py (device): the worked example of CIDEr-D / ROUGE-L and a random
corpus built to repeat n-grams."""
import numpy as np

#: the worked example: references without START / END, hypotheses, and the scores computed in fp64 from the definitions
REFS = [[[5, 6, 7, 8, 9], [5, 6, 7, 10]], [[5, 6, 11, 12], [5, 6, 11, 12]], [[13, 14, 5, 6, 7, 8], [9, 9, 9]], [[5, 20], [21]]]
HYPS = [[5, 6, 7, 8], [5, 6, 6, 11, 12, 12, 30], [9, 9], []]
CIDER = [4.2840811316265395, 3.3712563873866013, 2.465517791859791, 0.0]
ROUGE = [0.8714285714285713, 0.7648902821316614, 0.7721518987341772, 0.0]
CIDER_MEAN = 2.530213827718233


def random_corpus(B=37, R=5, T=24, vocab=12, seed=11):
    """``(refs, hyps)``: ``vocab`` tokens only, so that n-grams repeat, an n-gram reaches every image and references are duplicated
    (as the preprocessing fills R); reference lengths from 0 (stored length 1: START only) to T - 1 (stored length T), hypothesis
    lengths 0..T - 1, one hypothesis with term frequencies above its reference's."""
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
        hyps.append(rs.randint(0, vocab, size=b % T).tolist() if b % 4 else list(rr[b % R][:T - 1]))
    hyps[1] = (refs[1][0][:3] * 3)[:T - 1]
    hyps[2] = []
    return refs, hyps
