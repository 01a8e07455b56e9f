"""CPU: the host half of the on-device evaluation (sat_amd/evaluation.py): BLEU / GLEU from summed statistics against the
existing corpus functions, the random search's draws against the notebook's order, the C ABI's argument checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import caption_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd")


def all_corpora(golden_dir):
    c = dict(R.random_corpora())
    c.update(R.g10_corpora(golden_dir))
    c.update(R.edge_corpora())
    return c


def test_from_stats_equal_the_corpus_functions(golden_dir):
    """bleu_from_stats / gleu_from_stats of the per-segment statistics summed over a corpus == corpus_bleu / corpus_gleu, exactly"""
    import sat_amd  # noqa: F401
    from sat_amd import metrics
    checked = 0
    for name, (refs, caps) in all_corpora(golden_dir).items():
        tot = np.array(R.corpus_stats(refs, caps), np.int64).sum(0).tolist()
        for w in R.WEIGHTS:
            assert metrics.bleu_from_stats(tot[0:4], tot[4:8], tot[8], tot[9], w) == metrics.corpus_bleu(refs, caps, weights=w), (name, w)
            checked += 1
        assert metrics.gleu_from_stats(tot[10], tot[11]) == metrics.corpus_gleu(refs, caps), name
    assert checked >= 4 * 18
    # a corpus of several batches: the sums of the batches' statistics give the score of the concatenation
    refs, caps = [], []
    for r, c in R.random_corpora().values():
        refs += r; caps += c
    tot = np.array(R.corpus_stats(refs, caps), np.int64).sum(0).tolist()
    assert metrics.bleu_from_stats(tot[0:4], tot[4:8], tot[8], tot[9]) == metrics.corpus_bleu(refs, caps)
    assert metrics.bleu_from_stats([0, 0, 0, 0], [5, 4, 3, 2], 5, 5) == 0 and metrics.gleu_from_stats(0, 0) == 0.0


def test_reference_rules_of_the_statistics():
    """the hand-made cases say what they are meant to say (tests/caption_stats_ref.py)"""
    e = R.edge_corpora()
    assert R.corpus_stats(*e["hyp_empty"]) == [[0, 0, 0, 0, 1, 1, 1, 1, 0, 2, 0, 6], [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 3], [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]]
    a, b = R.corpus_stats(*e["repeat_once_and_twice"])
    assert a == b and a[0:2] == [4, 2]                       # unigrams 5, 6 twice each in the longer reference; bigram (5, 6) twice
    assert [s[9] for s in R.corpus_stats(*e["two_refs_equally_close"])] == [4, 4]
    assert [s[10:12] for s in R.corpus_stats(*e["equal_gleu_ratio"])] == [[1, 3], [2, 6]]
    assert [s[4:8] for s in R.corpus_stats(*e["hyp_shorter_than_n"])] == [[2, 1, 1, 1], [1, 1, 1, 1]]


class _StubModel:
    """records the decode parameters it is called with; returns fixed statistics (CPU tensors)"""

    def __init__(self):
        self.calls = []

    def val_batch_stats(self, batch, **decode):
        from sat_amd.evaluation import CaptionStats
        self.calls.append(decode)
        counts = torch.tensor([8, 5, 3, 2, 10, 9, 8, 7, 10, 11, 18, 34], dtype=torch.int64) * (1 + batch)
        return CaptionStats(counts, torch.tensor(1.5, dtype=torch.float64), torch.tensor(6.0, dtype=torch.float64), 2)


def test_random_search_draws_in_the_notebooks_order():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    for seed in (0, 7, 1234):
        model = _StubModel()
        rows = E.random_search(model, [0, 1, 2, 3, 4, 5], trials=6, seed=seed, max_batches=4)
        rs = np.random.RandomState(seed)
        assert len(rows) == 6 and len(model.calls) == 6 * 4
        for t, row in enumerate(rows):
            beamk = rs.choice([5, 20]); temperature = rs.uniform(0.7, 1.2); method = rs.choice(["beam", "multinomial"])
            noise = rs.choice([0.0]); rescore = rs.choice(["LN", "BAR"]); reward = rs.uniform(0.6, 1.3)
            assert (row["beamk"], row["temperature"], row["sample_method"], row["decoder_noise"], row["rescore_method"], row["rescore_reward"]) == \
                   (beamk, temperature, method, noise, rescore, reward)
            assert list(row)[:13] == E.HEADERS and all(k + "_corpus" in row for k in E.METRIC_KEYS)
            for call in model.calls[4 * t:4 * t + 4]:
                assert call["max_gen_length"] == 32 and call["beamk"] == beamk and call["temperature"] == temperature and call["rescore_reward"] == reward
                assert call["sample_method"] == method and call["rescore_method"] == rescore and call["decoder_noise"] == noise
    assert E.HEADERS == ["beamk", "temperature", "sample_method", "decoder_noise", "rescore_method", "rescore_reward", "bleu1", "bleu2", "bleu3", "bleu4",
                         "cosine_similarity", "gleu", "perplexity"]


def test_evaluate_batch_mean_and_corpus_on_host_numbers():
    """evaluate(): batch_mean is the plain mean of the per-batch dicts, corpus comes from the summed statistics; CaptionStats adds"""
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, metrics
    model = _StubModel()
    res = E.evaluate(model, [0, 1, 2], beamk=3)
    per = [model.val_batch_stats(b).metrics() for b in (0, 1, 2)]
    for k in E.METRIC_KEYS:
        assert res["batch_mean"][k] == sum(p[k] for p in per) / 3
    tot = model.val_batch_stats(0) + model.val_batch_stats(1) + model.val_batch_stats(2)
    assert tot.images == 6 and res["images"] == 6 and res["batches"] == 3
    assert res["corpus"] == tot.metrics()
    c = tot.counts.tolist()
    assert res["corpus"]["bleu4"] == metrics.bleu_from_stats(c[0:4], c[4:8], c[8], c[9]) and res["corpus"]["cosine_similarity"] == 4.5 / 6
    assert E.evaluate(model, [0, 1, 2], max_batches=2)["batches"] == 2


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "libsat_hip.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


def test_caption_scoring_exports_and_argument_checks(lib):
    """the three exports exist; null pointers and over-limit sizes return SAT_EINVAL (1) with text (no GPU is touched: every check
    comes before the launch)"""
    from sat_amd import _lib
    raw = ctypes.CDLL(os.path.join(PKG, "libsat_hip.so"))
    for name in ("sat_beam_select", "sat_caption_stats", "sat_caption_cosine"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS
    p = 4096                                                   # a non-null address: never dereferenced on the host, no launch follows
    sel = lambda **kw: lib.sat_beam_select(*[kw.get(k, p) for k in ("tok_in", "prev_row", "fin_count", "fin_step", "fin_row", "fin_score", "fin_mean", "alpha_hist")],
                                           kw.get("B", 2), kw.get("K", 3), kw.get("S", 8), kw.get("L", 4), kw.get("method", 1), 0.5, 0,
                                           *[kw.get(k, p) for k in ("cap_tokens", "cap_len", "cap_score", "cap_raw", "cap_step", "cap_alpha")], None)
    assert sel(tok_in=None) == 1 and b"null" in lib.sat_last_error()
    assert sel(cap_score=None) == 1 and b"null" in lib.sat_last_error()
    assert sel(alpha_hist=None) == 1 and b"alpha_hist" in lib.sat_last_error()          # maps asked for without the history
    assert sel(S=_lib.CAPTION_MAX_LEN) == 1 and b"limit" in lib.sat_last_error()
    assert sel(S=0) == 1 and sel(B=0) == 1 and b"non-positive" in lib.sat_last_error()
    assert sel(method=4) == 1 and b"rescore_method" in lib.sat_last_error()
    st = lambda **kw: lib.sat_caption_stats(kw.get("tok", p), kw.get("len", p), kw.get("W", 33), kw.get("refs", p), kw.get("rl", p), kw.get("B", 2),
                                            kw.get("R", 5), kw.get("T", 22), kw.get("stats", p), None)
    assert st(tok=None) == 1 and b"null" in lib.sat_last_error()
    assert st(stats=None) == 1 and b"null" in lib.sat_last_error()
    for over in (dict(W=_lib.CAPTION_MAX_LEN + 1), dict(T=_lib.CAPTION_MAX_LEN + 1), dict(R=_lib.CAPTION_MAX_REFS + 1)):
        assert st(**over) == 1 and b"over the limits" in lib.sat_last_error(), over
    assert st(R=0) == 1 and b"non-positive" in lib.sat_last_error()
    cs = lambda **kw: lib.sat_caption_cosine(kw.get("tok", p), p, kw.get("W", 33), p, p, 2, kw.get("R", 5), 22, kw.get("E", p), kw.get("V", 100),
                                             kw.get("m", 256), kw.get("best", p), None)
    assert cs(E=None) == 1 and b"null" in lib.sat_last_error()
    assert cs(best=None) == 1 and b"null" in lib.sat_last_error()
    assert cs(m=_lib.CAPTION_MAX_EMBED + 1) == 1 and b"limit" in lib.sat_last_error()
    assert cs(R=_lib.CAPTION_MAX_REFS + 1) == 1 and b"over the limits" in lib.sat_last_error()
    assert cs(V=0) == 1 and b"non-positive" in lib.sat_last_error()
    # the limits cover what the issue asks for at least
    assert _lib.CAPTION_MAX_LEN >= 65 and _lib.CAPTION_MAX_REFS >= 8
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    for name, val in (("SAT_CAPTION_MAX_LEN", _lib.CAPTION_MAX_LEN), ("SAT_CAPTION_MAX_REFS", _lib.CAPTION_MAX_REFS), ("SAT_CAPTION_MAX_EMBED", _lib.CAPTION_MAX_EMBED)):
        assert "#define %s %d\n" % (name, val) in header
