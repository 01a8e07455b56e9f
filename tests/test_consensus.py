"""CPU: CIDEr-D and ROUGE-L on the host (sat_amd/metrics.py: the specification of csrc/caption_consensus.hip) against the worked
example and hand-computed edge cases, the ``corpus=`` plumbing of sat_amd/evaluation.py on host numbers, and the checks that come
before any launch."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd")

from consensus_cases import CIDER, CIDER_MEAN, HYPS, REFS, ROUGE, random_corpus  # noqa: E402

#: two images without a common n-gram: every n-gram of a reference has df 1 and weighs log 2
TWO = [[[1, 2]], [[3, 4]]]


def _m():
    import sat_amd  # noqa: F401
    from sat_amd import metrics
    return metrics


def test_worked_example():
    m = _m()
    got = m.cider_d(REFS, HYPS)
    for b in range(4):
        assert abs(got[b] - CIDER[b]) <= 1e-12, (b, got[b])
        assert abs(m.rouge_l(REFS[b], HYPS[b]) - ROUGE[b]) <= 1e-12, b
    assert abs(sum(got) / 4 - CIDER_MEAN) <= 1e-12
    assert m.cider_d(REFS[:1], HYPS[:1]) == [0.0]                       # N = 1: log N = 0, every weight is 0
    df = m.document_frequency(REFS)
    assert m.cider_d(REFS, HYPS, df=df, n_images=4) == got
    with pytest.raises(ValueError):
        m.cider_d(REFS, HYPS, df=df)                                    # an explicit df needs its image count


def test_random_corpus_has_the_cases_it_is_meant_to_have():
    m = _m()
    refs, hyps = random_corpus()
    assert len(refs) == 37 and all(len(rr) == 5 for rr in refs)
    assert {len(h) for h in hyps} >= {0, 1, 23} and max(len(h) for h in hyps) == 23
    assert {len(r) for rr in refs for r in rr} >= {0, 23} and max(len(r) for rr in refs for r in rr) == 23
    df = m.document_frequency(refs)
    assert max(df.values()) == 37                                       # an n-gram of every image: weight 0
    assert any(rr[3] == rr[0] and len(rr[0]) > 0 for rr in refs)         # duplicated references
    assert any(n > 1 for n in df.values() if n < 37) and any(len(g) == 4 and n > 1 for g, n in df.items())
    scores = m.cider_d(refs, hyps)
    assert all(0.0 <= s <= 10.0 for s in scores) and scores[2] == 0.0 and max(scores) > 1.0


def test_document_frequency_counts_an_image_once():
    m = _m()
    assert m.document_frequency([[[1, 2], [1, 2]], [[1, 1]]]) == {(1,): 2, (2,): 1, (1, 2): 1, (1, 1): 1}
    df = m.document_frequency(REFS)
    assert df[(5,)] == 4 and df[(5, 6)] == 3 and df[(5, 6, 7)] == 2 and df[(5, 6, 7, 8)] == 2 and df[(9,)] == 2 and df[(9, 9, 9)] == 1
    assert df[(5, 6, 11, 12)] == 1                                      # the duplicated reference of image 2
    assert all(1 <= len(g) <= 4 for g in df)


def test_ngram_of_every_image_weighs_nothing():
    m = _m()
    refs = [[[5, 6]], [[5, 7]]]
    assert m.cider_d(refs, [[5], [5]]) == [0.0, 0.0]                    # the only common n-gram has df = N
    one = m.cider_d(refs, [[5, 6], [7]])
    # image 1: unigrams h {5: 0, 6: log 2} = r, bigram (5, 6) on both sides: two orders at 1, equal lengths
    assert abs(one[0] - 10 * 2 / 4) <= 1e-12
    # image 2: unigram 7 matches, r's norm is log 2 as well: 1; len_h = 0 against len_r = 1
    assert abs(one[1] - 10 * math.exp(-1 / 72) / 4) <= 1e-12


def test_unseen_ngram_weighs_tf_log_n():
    m = _m()
    # h = [1, 9]: 9 is in no reference (df 0 -> log N); it lengthens h's unigram norm to sqrt(2) log 2: the cosine is 1 / 2, not 1 / sqrt(2)
    got = m.cider_d(TWO, [[1, 9], [3, 4]])
    assert abs(got[0] - 10 * 0.5 / 4) <= 1e-12
    assert abs(got[1] - 10 * 2 / 4) <= 1e-12                            # the reference itself: orders 1 and 2 at 1, no 3- or 4-gram


def test_hypotheses_of_length_0_1_and_3():
    m = _m()
    pen = math.exp(-1 / 72)                                             # one bigram position apart, sigma = 6
    assert m.cider_d(TWO, [[], [3, 4]])[0] == 0.0
    assert abs(m.cider_d(TWO, [[1], [3, 4]])[0] - 10 * (1 / math.sqrt(2)) * pen / 4) <= 1e-12
    # [1, 2, 9]: unigrams 2 / sqrt(6), bigrams 1 / sqrt(2), the trigram meets no reference trigram (norm 0: no division)
    assert abs(m.cider_d(TWO, [[1, 2, 9], [3, 4]])[0] - 10 * (2 / math.sqrt(6) + 1 / math.sqrt(2)) * pen / 4) <= 1e-12
    assert m.rouge_l(TWO[0], []) == 0.0
    assert abs(m.rouge_l(TWO[0], [1]) - 2.44 * 1.0 * 0.5 / (0.5 + 1.44 * 1.0)) <= 1e-12
    assert abs(m.rouge_l(TWO[0], [1, 2, 9]) - 2.44 * (2 / 3) * 1.0 / (1.0 + 1.44 * (2 / 3))) <= 1e-12


def test_term_frequency_two_is_clipped_by_min():
    m = _m()
    # h = [1, 1, 2] against r = [1, 2]: w_h[1] = 2 log 2 is clipped to w_r[1] = log 2: dot = 2 log^2 2 (3 without the min)
    pen = math.exp(-1 / 72)
    want = 10 * (2 / math.sqrt(10) + 1 / math.sqrt(2)) * pen / 4
    assert abs(m.cider_d(TWO, [[1, 1, 2], [3, 4]])[0] - want) <= 1e-12


def test_rouge_l_empty_reference_and_separate_maxima():
    m = _m()
    assert m.rouge_l([[], [1, 2]], [1, 2]) == 1.0
    assert m.rouge_l([[]], [1]) == 0.0
    assert m.rouge_l([[3, 4]], [1, 2]) == 0.0
    assert m.lcs_length([1, 2, 3, 4, 5], [2, 9, 4, 5, 1]) == 3
    # precision comes from the long reference (LCS 3 of 3), recall from the short one (LCS 2 of 2)
    assert abs(m.rouge_l([[1, 2, 3, 7, 7, 7], [1, 2]], [1, 2, 3]) - 2.44 * 1.0 * 1.0 / (1.0 + 1.44 * 1.0)) <= 1e-12


class _StubModel:
    """fixed statistics (CPU tensors); scored against a corpus when one is passed, as SAT.val_batch_stats is"""

    def __init__(self):
        self.calls = []

    def val_batch_stats(self, batch, **decode):
        from sat_amd.evaluation import CaptionStats
        self.calls.append(decode)
        counts = torch.tensor([8, 5, 3, 2, 10, 9, 8, 7, 10, 11, 18, 34], dtype=torch.int64) * (1 + batch)
        consensus = torch.tensor([2.5, 1.25], dtype=torch.float64) * (1 + batch) if decode.get("corpus") is not None else None
        return CaptionStats(counts, torch.tensor(1.5, dtype=torch.float64), torch.tensor(6.0, dtype=torch.float64), 2, consensus)


def test_without_corpus_everything_is_as_before():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    model = _StubModel()
    st = model.val_batch_stats(0)
    assert st.vector().shape == (14,) and st.consensus_sum is None
    assert tuple(st.metrics()) == E.METRIC_KEYS
    res = E.evaluate(model, [0, 1, 2], beamk=3)
    assert tuple(res["batch_mean"]) == E.METRIC_KEYS and tuple(res["corpus"]) == E.METRIC_KEYS
    assert all("corpus" not in c for c in model.calls)
    rows = E.random_search(model, [0, 1, 2, 3], trials=2, seed=3)
    assert all(list(r) == E.HEADERS + [k + "_corpus" for k in E.METRIC_KEYS] for r in rows)
    assert all("corpus" not in c for c in model.calls)
    assert E.CONSENSUS_KEYS == ("cider", "rouge_l")


def test_with_a_corpus_the_two_keys_follow_the_existing_ones():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    model, corpus = _StubModel(), object()
    a, b = model.val_batch_stats(0, corpus=corpus), model.val_batch_stats(1, corpus=corpus)
    assert a.vector().shape == (16,) and a.vector().dtype == torch.float64
    assert a.vector()[:14].tolist() == model.val_batch_stats(0).vector().tolist()
    assert list(a.metrics()) == list(E.METRIC_KEYS) + ["cider", "rouge_l"]
    assert a.metrics()["cider"] == 2.5 / 2 and a.metrics()["rouge_l"] == 1.25 / 2
    tot = a + b
    assert tot.images == 4 and tot.consensus_sum.tolist() == [7.5, 3.75] and tot.metrics()["cider"] == 7.5 / 4
    for x, y in ((a, model.val_batch_stats(1)), (model.val_batch_stats(1), a)):
        with pytest.raises(ValueError):
            x + y
    res = E.evaluate(model, [0, 1, 2], corpus=corpus, beamk=3)
    assert list(res["batch_mean"]) == list(res["corpus"]) == list(E.METRIC_KEYS) + ["cider", "rouge_l"]
    assert all(c["corpus"] is corpus for c in model.calls[-3:])
    assert res["batch_mean"]["cider"] == (2.5 / 2 + 5.0 / 2 + 7.5 / 2) / 3 and res["corpus"]["cider"] == 15.0 / 6
    assert res["corpus"]["rouge_l"] == 7.5 / 6
    plain = E.evaluate(model, [0, 1, 2], beamk=3)
    assert all(res["batch_mean"][k] == plain["batch_mean"][k] and res["corpus"][k] == plain["corpus"][k] for k in E.METRIC_KEYS)
    rows = E.random_search(model, [0, 1, 2, 3], trials=2, seed=3, corpus=corpus)
    plain_rows = E.random_search(model, [0, 1, 2, 3], trials=2, seed=3)
    for r, p in zip(rows, plain_rows):
        assert list(r)[:13] == E.HEADERS
        assert list(r) == list(p) + ["cider", "rouge_l", "cider_corpus", "rouge_l_corpus"]
        assert all(r[k] == p[k] for k in p)


def test_reference_corpus_refuses_before_touching_a_gpu():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    with pytest.raises(ValueError, match="vocab_size"):
        E.ReferenceCorpus(65536)
    for cap in (0, 12, 1000):
        with pytest.raises(ValueError, match="power of two"):
            E.ReferenceCorpus(6400, capacity=cap)
    rc = E.ReferenceCorpus(65535, capacity=8)
    assert rc.capacity == 8 and rc.images == 0 and rc.to_dict() == {}
    # the default: the smallest power of two >= 2 x the announced n-gram positions; 5,000 images x 5 references of 12 words -> 2^22
    lengths = np.full((5000, 5), 13)                                   # START + 12 words: the reference is c[1:13]
    positions = E.ReferenceCorpus.positions(lengths)
    assert positions == 5000 * 5 * (12 + 11 + 10 + 9)
    assert E.ReferenceCorpus(6400, expected_positions=positions).capacity == 1 << 22
    assert E.ReferenceCorpus.positions([[1, 2, 3]]) == 0 + 1 + (2 + 1)   # START only, one word, two words
    assert E.ReferenceCorpus(6400, expected_positions=1024).capacity == 2048


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libsat_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


def test_consensus_exports_and_argument_checks(lib):
    """null pointers, sizes beyond the limits and a capacity that is no power of two return SAT_EINVAL (1) with text; every check
    comes before the launch, so no GPU is touched"""
    from sat_amd import _lib
    raw = ctypes.CDLL(os.path.join(PKG, "libsat_hip.so"))
    for name in ("sat_ngram_table_bytes", "sat_ngram_table_clear", "sat_ngram_table_add", "sat_caption_consensus"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS
    assert lib.sat_ngram_table_bytes(1 << 22) == 12 << 22 and lib.sat_ngram_table_bytes(1) == 12
    for cap in (0, -8, 12, (1 << 22) + 1):
        assert lib.sat_ngram_table_bytes(cap) == 0 and b"power of two" in lib.sat_last_error()
    p = 4096                                                            # a non-null address: never dereferenced on the host
    assert lib.sat_ngram_table_clear(None, 8, None) == 1 and b"null" in lib.sat_last_error()
    assert lib.sat_ngram_table_clear(p, 12, None) == 1 and b"power of two" in lib.sat_last_error()
    add = lambda **kw: lib.sat_ngram_table_add(kw.get("refs", p), kw.get("rl", p), kw.get("B", 2), kw.get("R", 5), kw.get("T", 22), kw.get("table", p),
                                               kw.get("cap", 64), kw.get("flag", p), None)
    for null in ("refs", "rl", "table", "flag"):
        assert add(**{null: None}) == 1 and b"null" in lib.sat_last_error(), null
    assert add(cap=48) == 1 and b"power of two" in lib.sat_last_error()
    assert add(R=_lib.CAPTION_MAX_REFS + 1) == 1 and b"over the limits" in lib.sat_last_error()
    assert add(T=_lib.CAPTION_MAX_LEN + 1) == 1 and b"over the limits" in lib.sat_last_error()
    assert add(B=0) == 1 and b"non-positive" in lib.sat_last_error()
    cs = lambda **kw: lib.sat_caption_consensus(kw.get("tok", p), kw.get("len", p), kw.get("W", 33), kw.get("refs", p), kw.get("rl", p), kw.get("B", 2),
                                                kw.get("R", 5), kw.get("T", 22), kw.get("table", p), kw.get("cap", 64), kw.get("N", 10),
                                                kw.get("sigma", 6.0), kw.get("scores", p), None)
    for null in ("tok", "len", "refs", "rl", "table", "scores"):
        assert cs(**{null: None}) == 1 and b"null" in lib.sat_last_error(), null
    for over in (dict(W=_lib.CAPTION_MAX_LEN + 1), dict(T=_lib.CAPTION_MAX_LEN + 1), dict(R=_lib.CAPTION_MAX_REFS + 1)):
        assert cs(**over) == 1 and b"over the limits" in lib.sat_last_error(), over
    assert cs(cap=100) == 1 and b"power of two" in lib.sat_last_error()
    assert cs(N=0) == 1 and b"n_images" in lib.sat_last_error()
    assert cs(sigma=0.0) == 1 and b"sigma" in lib.sat_last_error()
    assert cs(R=0) == 1 and b"non-positive" in lib.sat_last_error()
    lib.sat_abi_version.restype = ctypes.c_int
    assert lib.sat_abi_version() == 23                                  # symbols were added, nothing existing changed
