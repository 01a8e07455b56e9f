"""Cases shared by test_mbr.py (host) and test_gpu_mbr.py (device): the worked example of consensus reranking, beams of hypotheses over a
12-word vocabulary with the planted edge cases, and synthetic back-trace tables with their host walk."""
import numpy as np

from consensus_cases import random_corpus

#: the worked example (table: document_frequency(consensus_cases.REFS), n_images = 4), computed in fp64 from metrics.cider_d / rouge_l
HYPS = [[5, 6, 7, 8], [5, 6, 7, 10], [5, 6, 7, 8, 9], [13, 14], []]
LOGPS = [-2.0, -1.5, -3.0, -1.0, -4.0]
WORKED = [((1.0, 0.0), 0.0, [2.1420405658132697, 1.0535958198745439, 1.9260385633102224, 0.0, 0.0], 0),
          ((0.0, 1.0), 0.0, [0.40535714285714286, 0.3508928571428571, 0.39684014869888473, 0.0, 0.0], 0),
          ((0.5, 0.5), 1.0, [0.8173638877924871, 0.4910460278327679, 0.9831790903717652, 0.0, 0.0], 2)]

CIDER_TOL, ROUGE_TOL = 1e-9, 1e-12          # the project's tolerances for the two quantities (tests/test_gpu_consensus.py)
#: (K, width) of the kernel test: the smallest, an odd middle, the limits
SHAPES = [(2, 2), (5, 10), (32, 128)]
#: generator seed of ``beams``, chosen on the CPU with metrics.py alone: with it at least 3/4 of the non-degenerate images (two hypotheses
#: or more), taken over the three shapes together, keep their best and second-best host utility >= 1e-6 apart for every (reward, alpha) of
#: REWARDS (48 - 54 of 60 images; test_gpu_mbr.py asserts it from the host values)
BEAM_SEED = 7
REWARDS = [((1.0, 0.0), 0.0), ((0.0, 1.0), 0.0), ((0.5, 0.5), 1.0), ((1.0, 0.0), 1.0), ((0.0, 1.0), 1.0), ((0.5, 0.5), 0.0)]
GAP = 1e-6


def bound(reward, want):
    """per utility: a weighted mean cannot exceed its terms' error; the relative term covers the fp64 exp of the weights"""
    return reward[0] * CIDER_TOL + reward[1] * ROUGE_TOL + 1e-12 * abs(want)


def corpus_refs():
    """the references whose document frequencies the beams are scored with: consensus_cases.random_corpus (37 images, 12 words)"""
    return random_corpus()[0]


def beams(K, width, vocab=12, seed=BEAM_SEED):
    """``(hyps, logps)``: per image a list of at most K hypotheses (token lists of at most ``width`` of ``vocab`` words, so that
    n-grams repeat within and between hypotheses) and their raw scores.  Images 0..K have 0..K hypotheses; behind them the planted
    ones (and, for K >= 3, six full beams): exact duplicates (an exact tie: winner 0), an empty / a one-word / a full-width hypothesis
    side by side, a hypothesis whose term frequencies exceed its neighbour's (the ``min`` clipping), and siblings that share prefixes."""
    rs = np.random.RandomState(seed + 1000 * K + width)
    short = min(width, 12)                     # most hypotheses are caption-sized, so that the host reference stays quick

    def draw(n=None):
        n = rs.randint(0, short + 1) if n is None else n
        return rs.randint(0, vocab, size=n).tolist()

    hyps = [[draw() for _ in range(c)] for c in range(K + 1)]
    dup = draw(min(width, 5))
    hyps.append([list(dup) for _ in range(min(K, 3))])                                           # identical hypotheses
    hyps.append(([[], draw(1), draw(width), draw(width)] + [draw() for _ in range(K)])[:K])      # empty, one word, full width
    a = ([1, 1, 1, 2, 1, 1] * width)[:width]
    hyps.append(([a, [1, 2][:width], draw()] + [draw() for _ in range(K)])[:K])                  # tf above the neighbour's
    base = draw(min(width, 8))
    hyps.append([list(base)] + [list(base[:max(1, len(base) - 1 - (i % 3))]) + draw(min(i % 3, width - 1)) for i in range(K - 1)])   # siblings share prefixes
    if K >= 3:
        hyps += [[draw(rs.randint(2, short + 1)) for _ in range(K)] for _ in range(6)]           # full beams of ordinary captions
    logps = [(-rs.uniform(0.5, 9.0, size=len(h))).astype(np.float32).tolist() for h in hyps]
    return hyps, logps


def pack_beams(hyps, logps, K, width, pad=0):
    """-> numpy ``(hyp_tokens (B, K, width) int32, hyp_len (B, K) int32, counts (B) int32, logp (B, K) float32)``; the unused slots
    carry lengths and tokens that must not be read as hypotheses"""
    B = len(hyps)
    tok = np.full((B, K, width), pad, np.int32)
    ln, cnt, lp = np.zeros((B, K), np.int32), np.zeros(B, np.int32), np.zeros((B, K), np.float32)
    for b in range(B):
        cnt[b] = len(hyps[b])
        for f, h in enumerate(hyps[b]):
            tok[b, f, :len(h)] = h; ln[b, f] = len(h); lp[b, f] = logps[b][f]
        for f in range(len(hyps[b]), K):
            tok[b, f] = 3; ln[b, f] = width; lp[b, f] = 5.0          # a better raw score than any real one: must be ignored
    return tok, ln, cnt, lp


# ----------------------------------------------------------------------------- synthetic back-trace tables
def trace_tables(B, K, S, seed, vocab=83):
    """numpy tables in the layout of sat_beam_search_batched (tok_in / prev_row (S + 2, B, K), fin_count (B), fin_step / fin_row /
    fin_score (B, K)): fin_count runs 0..K over the images, fin_step 1..S; out-of-range steps and rows are planted in every unused
    slot, in the used slot (B - 1, 0) when it exists, and in the parent rows of image B - 2."""
    rs = np.random.RandomState(seed)
    tok_in = rs.randint(0, vocab, size=(S + 2, B, K)).astype(np.int32)
    prev_row = rs.randint(0, K, size=(S + 2, B, K)).astype(np.int32)
    fin_count = np.array([(b * K + B - 2) // (B - 1) if B > 1 else K for b in range(B)], np.int32)          # 0 .. K
    fin_count[B - 1] = K
    fin_step = rs.randint(1, S + 1, size=(B, K)).astype(np.int32)
    fin_step[0 if B == 1 else 1:, 0] = S                                                                     # the longest walk
    if K > 1:
        fin_step[:, 1] = 1                                                                                  # the shortest
    fin_row = rs.randint(0, K, size=(B, K)).astype(np.int32)
    fin_score = (-rs.uniform(0.5, 9.0, size=(B, K))).astype(np.float32)
    for b in range(B):
        for f in range(int(fin_count[b]), K):
            fin_step[b, f] = 10 ** 6 if f % 2 else -7
            fin_row[b, f] = -5 if f % 2 else K + 1000
    fin_step[B - 1, 0] = S + 50                    # used: clamped to S
    fin_row[B - 1, 0] = K + 7                      # used: clamped to K - 1
    if B > 1:
        prev_row[1::2, B - 2, :] = -3              # clamped to 0
        prev_row[2::2, B - 2, :] = K + 100         # clamped to K - 1
    return dict(tok_in=tok_in, prev_row=prev_row, fin_count=fin_count, fin_step=fin_step, fin_row=fin_row, fin_score=fin_score)


def host_trace(t, b, f, S, K):
    """the token list of finished slot (b, f): the walk of beam_select_kernel with its clamps"""
    step = int(np.clip(t["fin_step"][b, f], 0, S))
    cur = int(np.clip(t["fin_row"][b, f], 0, K - 1))
    out = [0] * step
    for s in range(step, 0, -1):
        out[s - 1] = int(t["tok_in"][s, b, cur])
        cur = int(np.clip(t["prev_row"][s, b, cur], 0, K - 1))
    return out
