"""CPU: chrF on the host (sat_amd/metrics.py: the specification of csrc/caption_chrf.hip) against the worked example, the kernel's
counting identity against collections.Counter, the host tables of ``evaluation.VocabChars``, the ``chrf=`` plumbing of
sat_amd/evaluation.py on host numbers, and the checks of sat_caption_chrf that come before any launch."""
import ctypes
import os
import subprocess
from collections import Counter

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd")

import chrf_cases as C  # noqa: E402


def _m():
    import sat_amd  # noqa: F401
    from sat_amd import metrics
    return metrics


def test_worked_example():
    m = _m()
    assert len(m.chrf_text(C.HYP)) == 14 and [len(m.chrf_text(r)) for r in C.REFS] == [15, 15, 19]
    for ref, stats, score in zip(C.REFS, C.STATS, C.SENTENCE):
        assert m.chrf_stats(ref, C.HYP) == stats
        assert abs(m.chrf_sentence(ref, C.HYP) - score) <= 1e-15
        assert abs(m.chrf_from_stats(*stats) - score) <= 1e-15
    assert abs(m.chrf(C.REFS, C.HYP) - C.IMAGE) <= 1e-15
    assert abs(m.chrf(C.REFS, C.HYP, beta=2.0) - C.IMAGE_BETA2) <= 1e-15
    assert m.chrf(C.REFS[::-1], C.HYP) == m.chrf(C.REFS, C.HYP)           # a maximum: the order of the references does not matter
    ref, hyp, rows, score = C.CAT
    tp, lh, lr = m.chrf_stats(ref, hyp)
    assert [(tp[n], max(lh - n, 0), max(lr - n, 0)) for n in range(6)] == rows
    assert abs(m.chrf_sentence(ref, hyp) - score) <= 1e-15
    assert abs(m.chrf_sentence(C.CAFE[0], C.CAFE[1]) - C.CAFE[2]) <= 1e-15           # code points count, not bytes
    assert m.chrf_sentence(C.HYP, C.HYP) == 1.0 and m.chrf([C.REFS[1], C.HYP], C.HYP) == 1.0
    for ref, hyp in ((C.HYP, []), ([], C.HYP), ([], [])):                 # an empty side: 1e-16 in every order
        assert abs(m.chrf_sentence(ref, hyp) - 1e-16) <= 1e-30
        assert m.chrf_stats(ref, hyp)[0] == [0] * 6


def test_text_strips_whitespace_and_keeps_code_points_whole():
    m = _m()
    assert m.chrf_text(["a", "man"]) == [ord(c) for c in "aman"]
    assert m.chrf_text(["skate board"]) == m.chrf_text(["skateboard"]) == m.chrf_text([" skate", "\tboard\n", " ", "　"])
    assert m.chrf_text(["café", "日本"]) == [99, 97, 102, 0xE9, 0x65E5, 0x672C]
    assert m.chrf_text(["\U0001F3C4"]) == [0x1F3C4] and m.chrf_text([]) == [] and m.chrf_text([7, 8]) == [55, 56]
    # what no token metric sees: one letter, one space
    assert m.chrf_sentence(["surfers"], ["surfer"]) > 0.5 and m.chrf_sentence(["skateboard"], ["skate", "board"]) == 1.0


def test_counting_identity_against_counter():
    """the walk of csrc/caption_chrf.hip (chrf_cases.walk_tp) gives sum over distinct n-grams of min(c_h, c_r) for every order"""
    m = _m()
    rs = np.random.RandomState(5)
    seen_more = seen_fewer = False
    for trial in range(300):
        hyp = C.spell(rs.randint(0, C.VOCAB_SIZE, size=rs.randint(0, 9)))
        ref = C.spell(rs.randint(0, C.VOCAB_SIZE, size=rs.randint(0, 9)))
        if trial % 10 == 0:
            hyp = (ref[:2] * 3)[:rs.randint(0, 7)]
        h, r = m.chrf_text(hyp), m.chrf_text(ref)
        want = []
        for n in range(1, 7):
            ch, cr = Counter(zip(*[h[k:] for k in range(n)])), Counter(zip(*[r[k:] for k in range(n)]))
            want.append(sum((ch & cr).values()))
            seen_more |= any(c > cr[g] > 0 for g, c in ch.items()); seen_fewer |= any(0 < c < cr[g] for g, c in ch.items())
        assert C.walk_tp(h, r) == want == m.chrf_stats(ref, hyp)[0], (hyp, ref)
    assert seen_more and seen_fewer
    assert C.walk_tp(m.chrf_text(C.HYP), m.chrf_text(C.REFS[2])) == C.STATS[2][0]


def test_corpus_chrf_is_the_mean_of_the_image_scores():
    m = _m()
    refs, hyps = C.random_corpus()
    refs, hyps = [[C.spell(r) for r in rr] for rr in refs[:12]], [C.spell(h) for h in hyps[:12]]
    scores = [m.chrf(rr, h) for rr, h in zip(refs, hyps)]
    assert m.corpus_chrf(refs, hyps) == sum(scores) / 12
    assert m.corpus_chrf(refs, hyps, beta=2.0) == sum(m.chrf(rr, h, 2.0) for rr, h in zip(refs, hyps)) / 12
    assert m.corpus_chrf([C.REFS], [C.HYP]) == m.chrf(C.REFS, C.HYP)
    with pytest.raises(AssertionError):
        m.corpus_chrf(refs, hyps[:3])


def test_random_corpus_has_the_cases_it_is_meant_to_have():
    m = _m()
    refs, hyps = C.random_corpus()
    assert len(refs) == 37 and all(len(rr) == 5 for rr in refs)
    assert {len(h) for h in hyps} == set(range(24))
    assert {len(r) for rr in refs for r in rr} >= {0, 23} and max(len(r) for rr in refs for r in rr) == 23
    assert any(rr[3] == rr[0] and len(rr[0]) > 0 for rr in refs)         # duplicated references
    hc = [len(m.chrf_text(C.spell(h))) for h in hyps]
    rc = [len(m.chrf_text(C.spell(r))) for rr in refs for r in rr]
    assert min(hc) == 0 and any(0 < n < 6 for n in hc) and max(hc) > 64   # orders without an n-gram; more than one wave
    assert min(rc) == 0 and any(0 < n < 6 for n in rc) and max(rc) > 64
    more = fewer = False
    for rr, h in zip(refs, hyps):
        ch = Counter(zip(*[m.chrf_text(C.spell(h))[k:] for k in range(3)]))
        for r in rr:
            cr = Counter(zip(*[m.chrf_text(C.spell(r))[k:] for k in range(3)]))
            more |= any(c > cr[g] > 0 for g, c in ch.items()); fewer |= any(0 < c < cr[g] for g, c in ch.items())
    assert more and fewer
    scores = [m.chrf([C.spell(r) for r in rr], C.spell(h)) for rr, h in zip(refs, hyps)]
    assert all(0.0 < s <= 1.0 for s in scores) and scores[0] < 1e-15 and any(s == 1.0 for s in scores) and any(0.1 < s < 0.9 for s in scores)


def test_vocab_chars_host_tables():
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, evaluation as E, metrics
    itos = {0: "<PAD>", 1: "a", 2: "skate board", 4: "日本", 5: "é", 7: ""}        # holes at 3 and 6; a space; an empty word
    offsets, chars, longest = E.VocabChars.host_tables(itos, 8)
    assert offsets.dtype == np.int32 and chars.dtype == np.int32 and isinstance(longest, int)
    spelled = ["<PAD>", "a", "skateboard", "<UNK>", "日本", "é", "<UNK>", ""]
    assert offsets.tolist() == np.cumsum([0] + [len(w) for w in spelled]).tolist() and longest == 10
    for i, w in enumerate(spelled):
        assert chars[offsets[i]:offsets[i + 1]].tolist() == [ord(c) for c in w] == metrics.chrf_text([w])
    assert len(chars) == offsets[-1] == sum(len(w) for w in spelled)
    # ids beyond the mapping spell <UNK> too; the tables of chrf_cases' vocabulary
    offsets, chars, longest = E.VocabChars.host_tables(C.VOCAB_ITOS, C.VOCAB_SIZE)
    assert chars[offsets[11]:offsets[12]].tolist() == [ord(c) for c in "<UNK>"] and longest == 6 and offsets[-1] == 33
    with pytest.raises(ValueError):
        E.VocabChars.host_tables({}, 0)
    with pytest.raises(L.SatHipError, match="GPU only"):                  # the tables live on the device: no CPU fallback
        E.VocabChars(C.VOCAB_ITOS, C.VOCAB_SIZE, device="cpu")
    assert E.CHRF_KEYS == ("chrf",) and (L.CHRF_MAX_ORDER, L.CHRF_MAX_CHARS) == (6, 2048)


COUNTS = [8, 5, 3, 2, 10, 9, 8, 7, 10, 11, 18, 34]


def test_metrics_from_vector_tells_the_four_lengths_apart():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    base = [float(c) for c in COUNTS] + [1.5, 6.0]
    plain = E.metrics_from_vector(base, 2)
    assert tuple(plain) == E.METRIC_KEYS
    with_chrf = E.metrics_from_vector(base + [0.75], 2)
    assert list(with_chrf) == list(E.METRIC_KEYS) + ["chrf"] and with_chrf["chrf"] == 0.375
    with_corpus = E.metrics_from_vector(base + [2.5, 1.25], 2)
    assert list(with_corpus) == list(E.METRIC_KEYS) + ["cider", "rouge_l"] and with_corpus["cider"] == 1.25 and with_corpus["rouge_l"] == 0.625
    both = E.metrics_from_vector(base + [2.5, 1.25, 0.75], 2)
    assert list(both) == list(E.METRIC_KEYS) + ["cider", "rouge_l", "chrf"]
    assert (both["cider"], both["rouge_l"], both["chrf"]) == (1.25, 0.625, 0.375)
    for d in (with_chrf, with_corpus, both):
        assert all(d[k] == plain[k] for k in E.METRIC_KEYS)
    for n in (13, 18):
        with pytest.raises(ValueError):
            E.metrics_from_vector((base + [0.0] * 4)[:n], 2)


class _StubModel:
    """fixed statistics (CPU tensors); scored against a corpus / with chrF when one is passed, as SAT.val_batch_stats is"""

    def __init__(self):
        self.calls = []

    def val_batch_stats(self, batch, **decode):
        from sat_amd.evaluation import CaptionStats
        self.calls.append(decode)
        counts = torch.tensor(COUNTS, dtype=torch.int64) * (1 + batch)
        consensus = torch.tensor([2.5, 1.25], dtype=torch.float64) * (1 + batch) if decode.get("corpus") is not None else None
        chrf = torch.tensor(0.75, dtype=torch.float64) * (1 + batch) if decode.get("chrf") is not None else None
        return CaptionStats(counts, torch.tensor(1.5, dtype=torch.float64), torch.tensor(6.0, dtype=torch.float64), 2, consensus, chrf)


def test_the_chrf_sum_travels_last():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    model, chars, corpus = _StubModel(), object(), object()
    plain, a, b = model.val_batch_stats(0), model.val_batch_stats(0, chrf=chars), model.val_batch_stats(1, chrf=chars)
    both = model.val_batch_stats(0, chrf=chars, corpus=corpus)
    assert plain.chrf_sum is None and plain.vector().shape == (14,)
    assert a.vector().shape == (15,) and both.vector().shape == (17,) and a.vector().dtype == torch.float64
    assert torch.equal(a.vector()[:14], plain.vector()) and torch.equal(both.vector()[:16], model.val_batch_stats(0, corpus=corpus).vector())
    assert a.vector()[14].item() == both.vector()[16].item() == 0.75
    assert list(a.metrics()) == list(E.METRIC_KEYS) + ["chrf"] and a.metrics()["chrf"] == 0.375
    tot = a + b
    assert tot.images == 4 and tot.chrf_sum.item() == 2.25 and tot.consensus_sum is None and tot.metrics()["chrf"] == 2.25 / 4
    assert (both + both).vector().shape == (17,)
    for x, y in ((a, plain), (plain, a), (both, model.val_batch_stats(0, corpus=corpus)), (a, both)):
        with pytest.raises(ValueError):
            x + y
    res = E.evaluate(model, [0, 1, 2], chrf=chars, chrf_beta=2.0, beamk=3)
    assert list(res["batch_mean"]) == list(res["corpus"]) == list(E.METRIC_KEYS) + ["chrf"]
    assert all(c["chrf"] is chars and c["chrf_beta"] == 2.0 and "corpus" not in c for c in model.calls[-3:])
    assert res["batch_mean"]["chrf"] == (0.75 / 2 + 1.5 / 2 + 2.25 / 2) / 3 and res["corpus"]["chrf"] == 4.5 / 6
    plain_res = E.evaluate(model, [0, 1, 2], beamk=3)
    assert all("chrf" not in c and "chrf_beta" not in c for c in model.calls[-3:])
    assert all(res[p][k] == plain_res[p][k] for p in ("batch_mean", "corpus") for k in E.METRIC_KEYS)
    res = E.evaluate(model, [0, 1, 2], chrf=chars, corpus=corpus, beamk=3)
    assert list(res["batch_mean"]) == list(res["corpus"]) == list(E.METRIC_KEYS) + ["cider", "rouge_l", "chrf"]
    assert res["corpus"]["chrf"] == 4.5 / 6 and res["corpus"]["cider"] == 15.0 / 6
    rows = E.random_search(model, [0, 1, 2, 3], trials=2, seed=3, chrf=chars)
    assert all(c["chrf"] is chars and c["chrf_beta"] == 3.0 for c in model.calls[-8:])
    plain_rows = E.random_search(model, [0, 1, 2, 3], trials=2, seed=3)
    both_rows = E.random_search(model, [0, 1, 2, 3], trials=2, seed=3, chrf=chars, corpus=corpus)
    for r, p, q in zip(rows, plain_rows, both_rows):
        assert list(r) == list(p) + ["chrf", "chrf_corpus"] and all(r[k] == p[k] for k in p)
        assert list(q) == list(p) + ["cider", "rouge_l", "cider_corpus", "rouge_l_corpus", "chrf", "chrf_corpus"]
        assert r["chrf"] == q["chrf"] == (0.75 / 2 + 1.5 / 2 + 2.25 / 2 + 3.0 / 2) / 4 and r["chrf_corpus"] == 7.5 / 8


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libsat_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


def test_chrf_export_and_argument_checks(lib):
    """null pointers, sizes beyond the limits, sentences that could exceed SAT_CHRF_MAX_CHARS and a beta that is not a positive finite
    number return SAT_EINVAL (1) with text; every check comes before the launch, so no GPU is touched"""
    from sat_amd import _lib
    raw = ctypes.CDLL(os.path.join(PKG, "libsat_hip.so"))
    assert hasattr(raw, "sat_caption_chrf") and "sat_caption_chrf" in _lib.SYMBOLS
    p = 4096                                                            # a non-null address: never dereferenced on the host
    names = ("tok", "len", "W", "refs", "rl", "B", "R", "T", "offsets", "chars", "V", "mwc", "beta", "scores", "stats")
    default = dict(tok=p, len=p, W=33, refs=p, rl=p, B=2, R=5, T=22, offsets=p, chars=p, V=6400, mwc=20, beta=3.0, scores=p, stats=None)

    def call(**kw):
        return lib.sat_caption_chrf(*[kw.get(n, default[n]) for n in names], None)

    for null in ("tok", "len", "refs", "rl", "offsets", "chars", "scores"):
        assert call(**{null: None}) == 1 and b"null" in lib.sat_last_error(), null
    for over in (dict(W=_lib.CAPTION_MAX_LEN + 1), dict(T=_lib.CAPTION_MAX_LEN + 1), dict(R=_lib.CAPTION_MAX_REFS + 1)):
        assert call(**over) == 1 and b"over the limits" in lib.sat_last_error(), over
    for zero in ("B", "R", "T", "W"):
        assert call(**{zero: 0}) == 1 and b"non-positive" in lib.sat_last_error(), zero
    assert call(B=-3) == 1 and b"non-positive" in lib.sat_last_error()
    assert call(V=0) == 1 and b"V=0" in lib.sat_last_error()
    assert call(mwc=-1) == 1 and b"max_word_chars" in lib.sat_last_error()
    # cap_width * max_word_chars and (T - 1) * max_word_chars against SAT_CHRF_MAX_CHARS, each on its own
    for sizes in (dict(W=128, T=22, mwc=17), dict(W=8, T=128, mwc=17), dict(W=33, T=22, mwc=63), dict(W=8, T=22, mwc=98), dict(W=1, T=2, mwc=2049),
                  dict(W=128, T=128, mwc=1 << 30)):
        assert call(**sizes) == 1 and b"characters" in lib.sat_last_error(), sizes
    for beta in (0.0, -3.0, float("inf"), float("nan")):
        assert call(beta=beta) == 1 and b"beta" in lib.sat_last_error(), beta
    lib.sat_abi_version.restype = ctypes.c_int
    assert lib.sat_abi_version() == 23                                  # a symbol was added, nothing existing changed
