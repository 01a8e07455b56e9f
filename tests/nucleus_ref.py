"""Nucleus (top-p) candidate selection restated in numpy float64 ("Sampled decoding"; include/sat_hip.h,
SAT_SAMPLE_NUCLEUS).  A helper for the tests, not a test module.

For one row of scores: F = the finite entries, w = exp(s - max_F s), W = sum_F w; F ordered by score descending, ties to the lower
id; the nucleus is the shortest leading run of that order whose weights sum to at least topp * W.  topp >= 1, or a running sum that
never reaches the target, gives all of F.  A non-empty F gives a non-empty nucleus."""
import numpy as np


def _ordered(scores_row):
    s = np.asarray(scores_row, dtype=np.float64)
    ids = np.nonzero(np.isfinite(s))[0]
    order = ids[np.lexsort((ids, -s[ids]))]          # primary: score descending; secondary: id ascending
    return s, order


def _cut(s, order, topp):
    """(cumulative weights, total, number of members)"""
    w = np.exp(s[order] - s[order].max())
    cum = np.cumsum(w)
    total = cum[-1]
    if topp >= 1.0:
        return cum, total, len(order)
    reach = np.nonzero(cum >= topp * total)[0]
    return cum, total, (int(reach[0]) + 1 if len(reach) else len(order))


def nucleus(scores_row, topp):
    """sorted member ids of the row's nucleus"""
    s, order = _ordered(scores_row)
    if len(order) == 0:
        return []
    _, _, count = _cut(s, order, float(topp))
    return sorted(int(v) for v in order[:count])


def boundary_margin(scores_row, topp):
    """The smallest |cumulative share - topp| over the cut position and its neighbour, the position before it: the distance by
    which rounding would have to move a partial sum for the member set to change.  Entries that tie with the entry at the cut
    count as ONE position (the tie rule, not a sum, decides among them): the shares compared are the one at the end of the run
    of equal scores and the one just before the run.  Where nothing is cut (topp >= 1, or no finite entry) the margin is inf."""
    s, order = _ordered(scores_row)
    topp = float(topp)
    if len(order) == 0 or topp >= 1.0:
        return float("inf")
    cum, total, count = _cut(s, order, topp)
    share = cum / total
    a = b = count - 1
    while a > 0 and s[order[a - 1]] == s[order[a]]:
        a -= 1
    while b + 1 < len(order) and s[order[b + 1]] == s[order[b]]:
        b += 1
    m = abs(share[b] - topp)
    if a > 0:
        m = min(m, abs(share[a - 1] - topp))
    return float(m)
