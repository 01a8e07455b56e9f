"""GPU: chrF on the device (csrc/caption_chrf.hip, evaluation.VocabChars, chrf_scores) against its host specification
(sat_amd/metrics.py: chrf_stats, chrf).

Tolerances.  The statistics (tp_1..tp_6, Lh, Lr) are integers and must be exact.  Scores within 1e-12 absolute: a score is at most 1 and
an image takes fewer than 100 fp64 roundings of 2^-53 (six F-scores of five operations each, their sum, one division), about 1e-14; the
mean over a batch adds one rounding per image."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chrf_cases as C  # noqa: E402
from test_gpu_consensus import _val_model, pack  # noqa: E402

TOL = 1e-12


def host(refs, hyps, itos, beta=3.0):
    """``(scores [B], stats [B][R][8])`` from metrics.py for token-id lists spelled by ``itos``"""
    from sat_amd import metrics
    scores, stats = [], []
    for rr, h in zip(refs, hyps):
        hw, rw = C.spell(h, itos), [C.spell(r, itos) for r in rr]
        scores.append(metrics.chrf(rw, hw, beta))
        stats.append([(lambda tp, lh, lr: tp + [lh, lr])(*metrics.chrf_stats(r, hw)) for r in rw])
    return scores, stats


def assert_close(got, want, label):
    got = got.cpu().tolist()
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert abs(g - w) <= TOL, (label, b, g, w)


@pytest.fixture(scope="module")
def random_corpus():
    """B = 37, R = 5, T = W = 24 over chrf_cases' twelve words; the host scores are computed once"""
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    refs, hyps = C.random_corpus(B=37, R=5, T=24)
    return dict(refs=refs, hyps=hyps, want=host(refs, hyps, C.VOCAB_ITOS), T=24, W=24, chars=E.VocabChars(C.VOCAB_ITOS, C.VOCAB_SIZE))


def test_worked_example():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, metrics
    itos, V, refs, hyp = C.example_ids()
    chars = E.VocabChars(itos, V)
    assert chars.word_offsets.dtype == chars.word_chars.dtype == torch.int32 and chars.word_offsets.is_cuda and chars.word_offsets.shape == (V + 1,)
    assert chars.max_word_chars == len("surfboard") and chars.vocab_size == V
    # image 0: the example; 1: the hypothesis among its references; 2: an empty hypothesis; 3: only empty references
    all_refs = [refs, [refs[1], hyp, refs[2]], refs, [[], [], []]]
    hyps = [hyp, hyp, [], hyp]
    tok, ln, rf, rl = pack(all_refs, hyps, T=8, W=6)
    got, stats = E.chrf_scores(tok, ln, rf, rl, chars, with_stats=True)
    assert got.shape == (4,) and got.dtype == torch.float64 and got.is_cuda and stats.shape == (4, 3, 8) and stats.dtype == torch.int32
    assert stats[0].tolist() == [tp + [lh, lr] for tp, lh, lr in C.STATS]
    assert_close(got, [C.IMAGE, 1.0, 1e-16, 1e-16], "worked example")
    assert got[1].item() == 1.0
    want, want_stats = host(all_refs, hyps, itos)
    assert stats.tolist() == want_stats
    assert_close(got, want, "worked example, host")
    assert torch.equal(E.chrf_scores(tok, ln, rf, rl, chars), got)        # without the statistics: the same scores
    # the single sentences, the first maximum among equal references, and the two small examples of the definition
    for r, score in enumerate(C.SENTENCE):
        one = pack([[refs[r]]], [hyp], T=8, W=6)
        assert abs(E.chrf_scores(*one, chars).item() - score) <= TOL
    for ref, hyp_w, score in (C.CAT[:2] + C.CAT[3:], C.CAFE):
        words = sorted(set(ref + hyp_w))
        small = E.VocabChars(dict(enumerate(words)), len(words))
        one = pack([[[words.index(w) for w in ref]]], [[words.index(w) for w in hyp_w]], T=4, W=3)
        s, st = E.chrf_scores(*one, small, with_stats=True)
        assert abs(s.item() - score) <= TOL, (ref, hyp_w, s.item())
        tp, lh, lr = metrics.chrf_stats(ref, hyp_w)
        assert st[0, 0].tolist() == tp + [lh, lr]
    assert st[0, 0].tolist() == [5, 3, 1, 0, 0, 0, 6, 6]                  # "cafe日本" against "café日本": code points, not bytes


def test_random_corpus_against_the_host(random_corpus):
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    c = random_corpus
    tok, ln, rf, rl = pack(c["refs"], c["hyps"], c["T"], c["W"])
    got, stats = E.chrf_scores(tok, ln, rf, rl, c["chars"], with_stats=True)
    assert stats.tolist() == c["want"][1]
    assert_close(got, c["want"][0], "random")
    assert torch.equal(E.chrf_scores(tok, ln, rf, rl, c["chars"]), got)   # two eager runs: the same bits


def test_beta(random_corpus):
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    itos, V, refs, hyp = C.example_ids()
    got = E.chrf_scores(*pack([refs], [hyp], T=8, W=6), E.VocabChars(itos, V), beta=2.0)
    assert abs(got.item() - C.IMAGE_BETA2) <= TOL
    c = random_corpus
    sub = slice(20, 30)
    tok, ln, rf, rl = pack(c["refs"][sub], c["hyps"][sub], c["T"], c["W"])
    assert_close(E.chrf_scores(tok, ln, rf, rl, c["chars"], beta=0.5), host(c["refs"][sub], c["hyps"][sub], C.VOCAB_ITOS, 0.5)[0], "beta 0.5")


def test_at_the_limits():
    """cap_width = 128 tokens of a 16-character word: a hypothesis of exactly SAT_CHRF_MAX_CHARS = 2048 characters, every loop strides
    beyond the workgroup and the "earlier positions" counts reach their largest values; T = 128 holds references of at most 127 tokens
    (SAT_CAPTION_MAX_LEN), 2032 characters.  R = 16, the extreme ids 0 and V - 1, and ids outside [0, V), which score as if absent."""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, evaluation as E
    words = ["abcdefghijklmnop", "ponmlkjihgfedcba", "ab", "a", "cdefgh", "", "abcdefghijklmnoq"]
    itos, V = dict(enumerate(words)), len(words)
    chars = E.VocabChars(itos, V)
    assert chars.max_word_chars == 16
    rs = np.random.RandomState(9)
    R, T = L.CAPTION_MAX_REFS, L.CAPTION_MAX_LEN
    long_ids = np.array([0, 1, V - 1])
    refs = [[(long_ids[rs.randint(0, 3, size=T - 1)] if r % 2 == 0 else rs.randint(0, V, size=rs.randint(0, T))).tolist() for r in range(R)]
            for _ in range(3)]
    hyps = [long_ids[rs.randint(0, 3, size=T)].tolist(), [0] * T, list(refs[2][0]) + [V - 1]]
    assert all(len(h) == T for h in hyps) and sum(len(words[t]) for t in hyps[0]) == L.CHRF_MAX_CHARS
    tok, ln, rf, rl = pack(refs, hyps, T, T, start=V - 1)
    want, want_stats = host(refs, hyps, itos)
    got, stats = E.chrf_scores(tok, ln, rf, rl, chars, with_stats=True)
    assert stats.tolist() == want_stats
    assert stats[:, :, 6].max().item() == 2048 and stats[:, :, 7].max().item() == 2032
    assert_close(got, want, "limits")
    # ids outside the vocabulary contribute no character: -1 and V in place of the empty word
    empty = words.index("")
    dirty = [[[(-1 if i % 2 else V) if t == empty else t for i, t in enumerate(r)] for r in rr] for rr in refs]
    tok2, ln2, rf2, rl2 = pack(dirty, hyps, T, T, start=V - 1)
    assert not torch.equal(rf2, rf)
    tok2[1, 5], tok2[1, 77] = -1, V                                       # two tokens fewer than hyps[1]
    got2, stats2 = E.chrf_scores(tok2, ln2, rf2, rl2, chars, with_stats=True)
    hyps_less = [hyps[0], [0] * (T - 2), hyps[2]]
    want2, want_stats2 = host(refs, hyps_less, itos)
    assert stats2.tolist() == want_stats2
    assert_close(got2, want2, "out-of-range ids")
    # one more character per word at the same width is refused before any launch
    chars.max_word_chars = 17
    with pytest.raises(L.SatHipError, match="characters"):
        E.chrf_scores(tok, ln, rf, rl, chars)


def test_val_batch_stats_evaluate_and_random_search_with_chrf():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, metrics
    model, batch = _val_model()
    # the tiny model's vocabulary names only its special tokens: give the other ids words (id 7 stays a hole and spells <UNK>)
    itos = dict(model.hp.vocab_itos)
    itos.update({i: C.WORDS[i % len(C.WORDS)] + "xyz"[i % 3] * (i % 4) for i in range(1, 57) if i != 7})
    model.hp.vocab_itos = itos
    chars = E.VocabChars.from_model(model)
    assert chars.vocab_size == 60 and chars.word_offsets.device == model.embedding.weight.device
    loader = [batch(s) for s in (41, 51, 61)]
    kw = dict(beamk=3, max_gen_length=7, temperature=1.0, rescore_method="LN")
    rc = E.ReferenceCorpus(60)
    for b in loader:
        rc.add(b[1], b[2])
    rc.check()
    per_image = []
    for b in loader:
        refs = [[model.decode_seq(c[1:l]) for c, l in zip(r, b[2][i].tolist())] for i, r in enumerate(b[1].tolist())]
        tok, ln, _, _ = model.caption_tokens(b[0], **kw)
        hyps = [model.decode_seq(t[:n]) for t, n in zip(tok.tolist(), ln.tolist())]
        scores = [metrics.chrf(rr, h) for rr, h in zip(refs, hyps)]
        per_image += scores
        plain, with_chrf = model.val_batch_stats(b, **kw), model.val_batch_stats(b, chrf=chars, **kw)
        with_corpus, both = model.val_batch_stats(b, corpus=rc, **kw), model.val_batch_stats(b, corpus=rc, chrf=chars, **kw)
        assert plain.vector().shape == (14,) and with_chrf.vector().shape == (15,) and both.vector().shape == (17,)
        assert torch.equal(with_chrf.vector()[:14], plain.vector()) and torch.equal(both.vector()[:16], with_corpus.vector())
        assert abs(with_chrf.metrics()["chrf"] - metrics.corpus_chrf(refs, hyps)) <= TOL
        assert both.metrics()["chrf"] == with_chrf.metrics()["chrf"]
        assert all(with_chrf.metrics()[k] == plain.metrics()[k] for k in E.METRIC_KEYS)
        beta2 = model.val_batch_stats(b, chrf=chars, chrf_beta=2.0, **kw).metrics()["chrf"]
        assert abs(beta2 - metrics.corpus_chrf(refs, hyps, beta=2.0)) <= TOL and beta2 != with_chrf.metrics()["chrf"]
        for x, y in ((plain, with_chrf), (with_chrf, plain), (with_corpus, both)):
            with pytest.raises(ValueError):
                x + y
        assert (with_chrf + with_chrf).vector().shape == (15,)
    assert 0.0 < min(per_image) and max(per_image) < 1.0 and len(set(per_image)) > 1        # the spelling makes the scores differ
    res, plain = E.evaluate(model, loader, chrf=chars, **kw), E.evaluate(model, loader, **kw)
    for part in ("batch_mean", "corpus"):
        assert list(res[part]) == list(E.METRIC_KEYS) + ["chrf"] and list(plain[part]) == list(E.METRIC_KEYS)
        assert all(res[part][k] == plain[part][k] for k in E.METRIC_KEYS)
        assert abs(res[part]["chrf"] - sum(per_image) / 12) <= TOL          # equal batch sizes: the same mean
    both = E.evaluate(model, loader, chrf=chars, corpus=rc, **kw)
    assert list(both["corpus"]) == list(E.METRIC_KEYS) + ["cider", "rouge_l", "chrf"] and both["corpus"]["chrf"] == res["corpus"]["chrf"]
    space = dict(E.NOTEBOOK_SPACE, beamks=[2, 3], sample_methods=["beam"], max_gen_length=7)
    rows = E.random_search(model, loader, trials=2, space=space, seed=3, max_batches=2, chrf=chars)
    plain_rows = E.random_search(model, loader, trials=2, space=space, seed=3, max_batches=2)
    for r, p in zip(rows, plain_rows):
        assert list(r) == list(p) + ["chrf", "chrf_corpus"] and all(r[k] == p[k] for k in p)
        assert 0.0 < r["chrf"] < 1.0 and abs(r["chrf"] - r["chrf_corpus"]) <= TOL


def test_scoring_runs_under_stream_capture(random_corpus):
    """chrf_scores captured into a graph and replayed, also for other references in the static input: bit-equal to the eager calls.
    A hidden synchronisation, allocation or host read would fail the capture."""
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    c = random_corpus
    tok, ln, rf, rl = pack(c["refs"], c["hyps"], c["T"], c["W"])
    other = [torch.roll(t, 5, 0).contiguous() for t in (rf, rl)]       # the references of other images: other scores
    eager = {"same": E.chrf_scores(tok, ln, rf, rl, c["chars"]).clone(), "other": E.chrf_scores(tok, ln, other[0], other[1], c["chars"]).clone()}
    assert torch.equal(E.chrf_scores(tok, ln, rf, rl, c["chars"]), eager["same"]) and not torch.equal(eager["same"], eager["other"])
    static = [rf.clone(), rl.clone()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, stats = E.chrf_scores(tok, ln, static[0], static[1], c["chars"], with_stats=True)
    for name, (a, l) in (("same", (rf, rl)), ("other", other), ("same", (rf, rl))):
        static[0].copy_(a); static[1].copy_(l)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[name]), name
    assert stats.tolist() == c["want"][1]
