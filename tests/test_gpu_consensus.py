"""GPU: the n-gram document-frequency table and CIDEr-D / ROUGE-L on the device (csrc/caption_consensus.hip, evaluation.ReferenceCorpus,
consensus_scores) against their host specification (sat_amd/metrics.py).

Tolerances.  CIDEr-D within 1e-9 absolute: scores are <= 10, an image sums at most 4 x 16 x 127 fp64 terms of a few roundings of 2^-53
each (below 1e-11), and 1e-9 leaves room for the device's log / exp differing from the host's in the last place.  ROUGE-L within
1e-12: integers (LCS, lengths) and five fp64 operations.  The table is compared as a dictionary, exactly."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import consensus_cases  # noqa: E402
from consensus_cases import CIDER, HYPS, REFS, ROUGE  # noqa: E402

CIDER_TOL, ROUGE_TOL = 1e-9, 1e-12


def pack(refs, hyps, T, W, start=1):
    """token lists -> (tokens (B, W), lengths (B), refs (B, R, T) with START in column 0, ref_lengths (B, R)) as int32 device tensors"""
    B, R = len(refs), len(refs[0])
    tok, ln = np.zeros((B, W), np.int32), np.zeros(B, np.int32)
    rf, rl = np.zeros((B, R, T), np.int32), np.zeros((B, R), np.int32)
    for b in range(B):
        tok[b, :len(hyps[b])] = hyps[b]; ln[b] = len(hyps[b])
        for r in range(R):
            rf[b, r, 0] = start
            rf[b, r, 1:1 + len(refs[b][r])] = refs[b][r]; rl[b, r] = 1 + len(refs[b][r])
    return [torch.from_numpy(a).cuda() for a in (tok, ln, rf, rl)]


def host_scores(refs, hyps, df=None, n_images=None):
    from sat_amd import metrics
    return metrics.cider_d(refs, hyps, df=df, n_images=n_images), [metrics.rouge_l(r, h) for r, h in zip(refs, hyps)]


def assert_scores(got, want, label):
    got = got.cpu().tolist()
    for b, (c, r) in enumerate(zip(*want)):
        assert abs(got[b][0] - c) <= CIDER_TOL, (label, b, "cider", got[b][0], c)
        assert abs(got[b][1] - r) <= ROUGE_TOL, (label, b, "rouge_l", got[b][1], r)


@pytest.fixture(scope="module")
def random_corpus():
    """B = 37, R = 5, T = 24, 12 tokens: n-grams repeat, df reaches N, references are duplicated; hypothesis lengths 0..23, reference
    lengths from 1 (START only: an empty reference) to T.  The host scores are computed once."""
    import sat_amd  # noqa: F401
    from sat_amd import metrics
    refs, hyps = consensus_cases.random_corpus(B=37, R=5, T=24, vocab=12)
    return dict(refs=refs, hyps=hyps, df=metrics.document_frequency(refs), want=host_scores(refs, hyps), T=24, W=24)


def build(refs, T, vocab=65535, capacity=None, splits=None):
    from sat_amd import evaluation as E
    _, _, rf, rl = pack(refs, [[] for _ in refs], T, 1)
    rc = E.ReferenceCorpus(vocab, capacity=capacity, expected_positions=E.ReferenceCorpus.positions(rl.cpu()))
    lo = 0
    for n in splits or [len(refs)]:
        rc.add(rf[lo:lo + n], rl[lo:lo + n]); lo += n
    assert lo == len(refs) and rc.images == len(refs)
    return rc


def test_worked_example():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, metrics
    tok, ln, rf, rl = pack(REFS, HYPS, T=8, W=8)
    rc = E.ReferenceCorpus(40).add(rf, rl).check()
    assert rc.images == 4 and rc.to_dict() == metrics.document_frequency(REFS)
    got = E.consensus_scores(tok, ln, rf, rl, rc)
    assert got.shape == (4, 2) and got.dtype == torch.float64 and got.is_cuda
    assert_scores(got, (CIDER, ROUGE), "worked example")
    assert got[3].tolist() == [0.0, 0.0]                               # the empty hypothesis
    one = E.ReferenceCorpus(40).add(rf[:1], rl[:1]).check()
    assert E.consensus_scores(tok[:1], ln[:1], rf[:1], rl[:1], one)[0, 0].item() == 0.0           # N = 1
    # host tensors of another integer dtype build the same table
    assert E.ReferenceCorpus(40).add(rf.cpu().long(), rl.cpu().to(torch.int16)).to_dict() == rc.to_dict()
    with pytest.raises(ValueError):
        E.consensus_scores(tok, ln, rf, rl, E.ReferenceCorpus(40))
    # a dataset's nested lists, fed in chunks of 3 + 1 images
    ds = types.SimpleNamespace(encoded_captions=rf.cpu().tolist(), lengths=rl.cpu().tolist(), vocab_stoi={str(i): i for i in range(40)})
    chunks = E.ReferenceCorpus.from_dataset(ds, chunk=3).check()
    assert chunks.images == 4 and chunks.vocab_size == 40 and chunks.to_dict() == rc.to_dict()
    assert chunks.capacity == E._pow2_at_least(2 * E.ReferenceCorpus.positions(rl.cpu()))
    assert torch.equal(E.consensus_scores(tok, ln, rf, rl, chunks), got)


def test_random_corpus_against_the_host(random_corpus):
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    c = random_corpus
    rc = build(c["refs"], c["T"], vocab=12).check()
    assert rc.to_dict() == c["df"]
    tok, ln, rf, rl = pack(c["refs"], c["hyps"], c["T"], c["W"])
    assert_scores(E.consensus_scores(tok, ln, rf, rl, rc), c["want"], "random")


def test_at_the_limits():
    """R = 16, T = W = 128 and the extreme token ids: the key's 16-bit fields are full, the LCS row is full"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, evaluation as E, metrics
    rs = np.random.RandomState(5)
    ids = np.array([0, 1, 65533, 65534])
    R, T = L.CAPTION_MAX_REFS, L.CAPTION_MAX_LEN
    refs = [[ids[rs.randint(0, 4, size=T - 1 if r % 2 == 0 else rs.randint(1, T))].tolist() for r in range(R)] for _ in range(3)]
    hyps = [ids[rs.randint(0, 4, size=T)].tolist(), list(refs[1][0]) + [65534], ids[rs.randint(0, 4, size=T // 2 + 1)].tolist()]
    assert len(hyps[0]) == len(hyps[1]) == T
    tok, ln, rf, rl = pack(refs, hyps, T, T, start=65532)
    rc = E.ReferenceCorpus(65535, expected_positions=E.ReferenceCorpus.positions(rl.cpu())).add(rf, rl).check()
    assert rc.to_dict() == metrics.document_frequency(refs)
    assert_scores(E.consensus_scores(tok, ln, rf, rl, rc), host_scores(refs, hyps), "limits")


def test_crowded_table_incremental_build_and_rebuild(random_corpus):
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    c = random_corpus
    tok, ln, rf, rl = pack(c["refs"], c["hyps"], c["T"], c["W"])
    roomy = build(c["refs"], c["T"]).check()
    base = E.consensus_scores(tok, ln, rf, rl, roomy)
    # the smallest power of two above the number of distinct n-grams: long probe chains
    crowded = build(c["refs"], c["T"], capacity=E._pow2_at_least(len(c["df"]) + 1)).check()
    assert len(c["df"]) < crowded.capacity <= 2 * len(c["df"]) and crowded.capacity < roomy.capacity
    assert crowded.to_dict() == c["df"]
    got = E.consensus_scores(tok, ln, rf, rl, crowded)
    assert_scores(got, c["want"], "crowded")
    assert torch.equal(got, base)                                      # the same content gives the same bits, wherever the slots are
    # three adds of 13 + 13 + 11 images
    parts = build(c["refs"], c["T"], splits=[13, 13, 11]).check()
    assert parts.to_dict() == c["df"]
    assert torch.equal(E.consensus_scores(tok, ln, rf, rl, parts), base)
    # build and score again
    again = build(c["refs"], c["T"]).check()
    assert again.to_dict() == c["df"]
    assert torch.equal(E.consensus_scores(tok, ln, rf, rl, again), base)
    # clear() starts over in place
    roomy.clear()
    assert roomy.images == 0
    roomy.add(rf, rl).check()
    assert roomy.to_dict() == c["df"] and torch.equal(E.consensus_scores(tok, ln, rf, rl, roomy), base)


def test_overflow_is_reported_and_harmless():
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, evaluation as E, metrics
    df = metrics.document_frequency(REFS)
    assert len(df) > 8
    tok, ln, rf, rl = pack(REFS, HYPS, T=8, W=8)
    small = E.ReferenceCorpus(40, capacity=8).add(rf, rl)
    torch.cuda.synchronize()                                           # the launch completes
    with pytest.raises(L.SatHipError, match="overflow"):
        small.check()
    held = small.to_dict()
    assert len(held) == 8 and all(g in df and 1 <= n <= df[g] for g, n in held.items())
    fresh = E.ReferenceCorpus(40).add(rf, rl).check()
    assert fresh.to_dict() == df
    assert_scores(E.consensus_scores(tok, ln, rf, rl, fresh), (CIDER, ROUGE), "after overflow")


def test_scoring_a_batch_of_a_larger_corpus(random_corpus):
    """the table holds 37 images, a batch of 5 of them is scored: df and N come from the corpus, not from the batch"""
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    c = random_corpus
    rc = build(c["refs"], c["T"]).check()
    sub = [3, 8, 20, 21, 36]
    refs, hyps = [c["refs"][i] for i in sub], [c["hyps"][i] for i in sub]
    tok, ln, rf, rl = pack(refs, hyps, c["T"], c["W"])
    assert_scores(E.consensus_scores(tok, ln, rf, rl, rc), host_scores(refs, hyps, df=c["df"], n_images=37), "sub-batch")


def _val_model():
    """the tiny model and batch maker of test_gpu_evaluation.py"""
    from sat_amd import model as M
    from oracle import prng, sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16,
                decoder_dim=40, deep_output=True, val_beamk=3, val_max_len=7)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over))).cuda()

    def batch(seed):
        B, Rn, T = 4, 3, 9
        img = torch.from_numpy(prng.uniform((B, 3, 64, 64), seed, 0.0, 1.0))
        caps, lengths = prng.captions(B, Rn, T, 60, seed + 1, min_len=3)
        return img.cuda(), torch.from_numpy(caps).cuda(), torch.from_numpy(lengths)

    return model, batch


def test_val_batch_stats_and_evaluate_with_a_corpus():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, metrics
    model, batch = _val_model()
    loader = [batch(s) for s in (41, 51, 61)]
    kw = dict(beamk=3, max_gen_length=7, temperature=1.0, rescore_method="LN")
    rc = E.ReferenceCorpus(60)
    for b in loader:
        rc.add(b[1], b[2])
    rc.check()
    refs = [[[c[1:l] for c, l in zip(r, b[2][i].tolist())] for i, r in enumerate(b[1].tolist())] for b in loader]
    df = metrics.document_frequency([r for rb in refs for r in rb])
    assert rc.images == 12 and rc.to_dict() == df
    ciders = []
    for b, rb in zip(loader, refs):
        tok, ln, _, _ = model.caption_tokens(b[0], **kw)
        hyps = [t[:n] for t, n in zip(tok.tolist(), ln.tolist())]
        cider, rouge = host_scores(rb, hyps, df=df, n_images=12)
        ciders += cider
        with_corpus, without, default = model.val_batch_stats(b, corpus=rc, **kw), model.val_batch_stats(b, corpus=None, **kw), model.val_batch_stats(b, **kw)
        got = with_corpus.metrics()
        assert abs(got["cider"] - sum(cider) / 4) <= CIDER_TOL and abs(got["rouge_l"] - sum(rouge) / 4) <= ROUGE_TOL
        assert default.vector().shape == (14,) and with_corpus.vector().shape == (16,)
        assert torch.equal(without.vector(), default.vector()) and torch.equal(with_corpus.vector()[:14], default.vector())
        assert set(default.metrics()) == set(E.METRIC_KEYS) and all(got[k] == default.metrics()[k] for k in E.METRIC_KEYS)
    res, plain = E.evaluate(model, loader, corpus=rc, **kw), E.evaluate(model, loader, **kw)
    assert res["images"] == 12 and abs(res["corpus"]["cider"] - sum(ciders) / 12) <= CIDER_TOL
    assert abs(res["batch_mean"]["cider"] - sum(ciders) / 12) <= CIDER_TOL                       # equal batch sizes: the same mean
    assert set(plain["corpus"]) == set(E.METRIC_KEYS)
    assert all(res[p][k] == plain[p][k] for p in ("batch_mean", "corpus") for k in E.METRIC_KEYS)


def test_build_and_scoring_run_under_stream_capture(random_corpus):
    """clear + add + consensus_scores captured into a graph and replayed, also for other references in the static input: bit-equal
    to the eager calls.  A hidden synchronisation, allocation or host read would fail the capture."""
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    c = random_corpus
    tok, ln, rf, rl = pack(c["refs"], c["hyps"], c["T"], c["W"])
    other = [torch.roll(t, 5, 0).contiguous() for t in (rf, rl)]       # the references of other images: another table, other scores
    eager, tables = {}, {}
    for name, (a, l) in (("same", (rf, rl)), ("other", other)):
        rc = E.ReferenceCorpus(12, capacity=1 << 14).add(a, l).check()
        eager[name], tables[name] = E.consensus_scores(tok, ln, a, l, rc).clone(), rc.to_dict()
    assert not torch.equal(eager["same"], eager["other"])
    static = [rf.clone(), rl.clone()]
    rc = E.ReferenceCorpus(12, capacity=1 << 14).clear()               # allocated before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc.clear().add(static[0], static[1])
        out = E.consensus_scores(tok, ln, static[0], static[1], rc)
    for name, (a, l) in (("same", (rf, rl)), ("other", other), ("same", (rf, rl))):
        static[0].copy_(a); static[1].copy_(l)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[name]), name
        assert rc.check().to_dict() == tables[name], name
