"""GPU: sat_caption_diversity and sat_caption_vocab_usage ("Beam diversity") against their host specification
(sat_amd/metrics.py: diversity_stats, diversity_per_hypothesis; numpy.bincount), then the statistics behind the batched search:
evaluate(..., with_diversity=True) against the specification applied to the finished hypotheses read back.

No tolerance anywhere: every compared quantity is an integer, or a float computed on the host from equal integers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diversity_cases as DC  # noqa: E402
import test_gpu_consensus as TG  # noqa: E402

SENTINEL, GUARD = -777, 64


def _metrics():
    import sat_amd  # noqa: F401
    from sat_amd import metrics
    return metrics


def _device_beams(K, W):
    hyps = DC.beams(K, W)
    return hyps, [torch.from_numpy(a).cuda() for a in DC.pack(hyps, K, W)]


def _raw(tok, ln, cnt, with_per_hyp):
    """the C entry on guarded buffers: ``(stats (B, 20), per_hyp (B, K, 10) or None)`` as numpy, the guard bands checked"""
    from sat_amd import _lib as L
    B, K, W = tok.shape
    st_buf = torch.full((GUARD + B * 20 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    ph_buf = torch.full((GUARD + B * K * 10 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    L.check(L.lib().sat_caption_diversity(L.ptr(tok), L.ptr(ln), L.ptr(cnt), B, K, W, L.ptr(st_buf[GUARD:]), L.ptr(ph_buf[GUARD:]) if with_per_hyp else None,
                                          L.stream_ptr()), "sat_caption_diversity")
    st, ph = st_buf.cpu().numpy(), ph_buf.cpu().numpy()
    assert (st[:GUARD] == SENTINEL).all() and (st[GUARD + B * 20:] == SENTINEL).all()
    if with_per_hyp:
        assert (ph[:GUARD] == SENTINEL).all() and (ph[GUARD + B * K * 10:] == SENTINEL).all()
    else:
        assert (ph == SENTINEL).all()
    return st[GUARD:GUARD + B * 20].reshape(B, 20), ph[GUARD:GUARD + B * K * 10].reshape(B, K, 10) if with_per_hyp else None


@pytest.mark.parametrize("K,W", DC.SHAPES)
def test_diversity_statistics_equal_the_host_specification(K, W):
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    hyps, (tok, ln, cnt) = _device_beams(K, W)
    want_stats, want_per = (torch.tensor(x, dtype=torch.int32) for x in DC.expected(K, W))
    stats, per_hyp = E.diversity_statistics(tok, ln, cnt, per_hypothesis=True)
    assert stats.shape == (len(hyps), 20) and per_hyp.shape == (len(hyps), K, 10) and stats.dtype == per_hyp.dtype == torch.int32
    got_stats, got_per = stats.cpu(), per_hyp.cpu()
    for b in np.nonzero((got_stats != want_stats).any(1).numpy())[0][:3]:
        print("K=%d W=%d image %d: device %s host %s" % (K, W, b, got_stats[b].tolist(), want_stats[b].tolist()))
    assert torch.equal(got_stats, want_stats)
    assert torch.equal(got_per, want_per)
    # without per_hyp: the same statistics
    only = E.diversity_statistics(tok, ln, cnt)
    assert torch.equal(only.cpu(), want_stats)
    # the same input gives the same bits
    again = E.diversity_statistics(tok, ln, cnt, per_hypothesis=True)
    assert torch.equal(again[0], stats) and torch.equal(again[1], per_hyp)
    # guard bands around both outputs stay untouched, with per_hyp and with NULL
    for with_per in (True, False):
        st, ph = _raw(tok, ln, cnt, with_per)
        assert np.array_equal(st, want_stats.numpy())
        assert ph is None or np.array_equal(ph, want_per.numpy())


def test_vocab_usage_equals_bincount():
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, evaluation as E
    rs = np.random.RandomState(5)
    for B, W, V in ((1, 1, 1), (7, 5, 11), (300, 33, 60), (64, 128, 6400)):
        tok = rs.randint(-3, V + 4, size=(B, W)).astype(np.int32)                   # ids on both sides of [0, V)
        ln = rs.randint(-2, W + 3, size=B).astype(np.int32)                         # lengths on both sides of [0, W]
        ln[0] = W
        tok[0, 0] = V                                                               # the first id outside
        used = np.concatenate([tok[b, :int(np.clip(ln[b], 0, W))] for b in range(B)])
        assert ((used < 0) | (used >= V)).any() and (ln > W).any() or B == 1
        want = np.bincount(used[(used >= 0) & (used < V)], minlength=V)
        d_tok, d_ln = torch.from_numpy(tok).cuda(), torch.from_numpy(ln).cuda()
        counts = E.vocabulary_usage(d_tok, d_ln, V)
        assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), want), (B, W, V)
        assert E.vocabulary_usage(d_tok, d_ln, V, counts) is counts                 # a second call accumulates
        assert np.array_equal(counts.cpu().numpy(), 2 * want), (B, W, V)
        buf = torch.full((GUARD + V + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        buf[GUARD:GUARD + V] = 0
        L.check(L.lib().sat_caption_vocab_usage(L.ptr(d_tok), L.ptr(d_ln), W, B, V, L.ptr(buf[GUARD:]), L.stream_ptr()), "sat_caption_vocab_usage")
        host = buf.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + V:] == SENTINEL).all() and np.array_equal(host[GUARD:GUARD + V], want)


def _host_diversity(model, loader, kw, search):
    """the specification applied to ``finished_hypotheses`` of every batch read back, and the words of the selected captions;
    every image's hypotheses are, as a multiset, what ``caption(..., return_all=True)`` returns"""
    from sat_amd import evaluation as E
    m = _metrics()
    sums, used, images = [0] * 20, set(), []
    for b in loader:
        model.eval()
        ann, _ = model.encode(b[0])
        o = model._beam_search_device(ann.contiguous(), kw["beamk"], kw["max_gen_length"], kw["temperature"], **search)
        hyp_tokens, hyp_len = E.finished_hypotheses(o, model.pad_idx)
        tok, ln, cnt = hyp_tokens.cpu().tolist(), hyp_len.cpu().tolist(), o["fin_count"].cpu().tolist()
        every = model.caption(b[0], return_all=True, **kw, **search)[0]
        for i in range(len(cnt)):
            hyps = [tok[i][f][:ln[i][f]] for f in range(cnt[i])]
            assert sorted(map(tuple, hyps)) == sorted(map(tuple, every[i])), i
            sums = [x + y for x, y in zip(sums, m.diversity_stats(hyps))]
            images.append(hyps)
        win, win_len, _, _ = model.caption_tokens(b[0], **kw, **search)
        for t, n in zip(win.cpu().tolist(), win_len.cpu().tolist()):
            used.update(t[:n])
    return sums, used, images


@pytest.mark.parametrize("search", [{}, {"beam_groups": 2}], ids=["plain", "groups"])
def test_evaluate_with_diversity_behind_the_batched_search(search):
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    m = _metrics()
    model, batch = TG._val_model()
    loader = [batch(s) for s in (41, 51)]
    kw = dict(beamk=4, max_gen_length=7, temperature=1.0, rescore_method="LN")
    off = E.evaluate(model, loader, **kw, **search)
    on = E.evaluate(model, loader, with_diversity=True, **kw, **search)
    assert set(off) == {"batch_mean", "corpus", "batches", "images"} and set(on) == set(off) | {"diversity"}
    for k in off:
        assert on[k] == off[k], k                                                   # dicts of floats: equal bit for bit
    sums, used, images = _host_diversity(model, loader, kw, search)
    want = m.diversity_from_stats(sums, vocab_used=len(used))
    print("%s: %s" % (search, on["diversity"]))
    assert on["diversity"] == want
    assert set(want) == set(m.DIVERSITY_KEYS) | {"vocabulary"} and want["hypotheses"] == sum(len(h) for h in images) > 8
    assert all(0 <= t < 60 for t in used) and want["vocabulary"] == len(used) >= 1
    # the batch form: the same columns, added on the device
    st = [model.val_batch_stats(b, with_diversity=True, **kw, **search) for b in loader]
    total = st[0] + st[1]
    assert st[0].diversity.images == 4 and total.diversity.images == 8 and total.diversity.vocab_size == 60
    assert total.diversity.sums.dtype == total.diversity.vocab_counts.dtype == torch.int64 and total.diversity.sums.is_cuda
    assert total.diversity.sums.cpu().tolist() == sums and total.diversity.metrics() == want
    assert total.vector().shape == (14,) and model.val_batch_stats(loader[0], **kw, **search).diversity is None
    with pytest.raises(ValueError, match="diversity"):
        st[0] + model.val_batch_stats(loader[1], **kw, **search)


def test_diversity_with_mbr_and_with_one_hypothesis_per_image():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    model, batch = TG._val_model()
    loader = [batch(s) for s in (41, 51)]
    kw = dict(beamk=4, max_gen_length=7, temperature=1.0)
    rc = E.ReferenceCorpus(60)
    for b in loader:
        rc.add(b[1], b[2])
    rc.check()
    # consensus reranking picks other winners among the same hypotheses: its back-trace is reused, the 20 sums are the plain search's
    plain = [model.val_batch_stats(b, with_diversity=True, rescore_method="LN", **kw) for b in loader]
    mbr = [model.val_batch_stats(b, with_diversity=True, rescore_method="MBR", mbr_corpus=rc, mbr_reward=(0.5, 0.5), **kw) for b in loader]
    for p, q in zip(plain, mbr):
        assert torch.equal(p.diversity.sums, q.diversity.sums) and int(q.diversity.sums[8]) > 4
    # pure sampling: one hypothesis per image, distinct-n and unique are defined, there is nothing to compare with
    res = E.evaluate(model, loader, with_diversity=True, sample_method="ancestral", beamk=1, max_gen_length=7, temperature=1.0, seed=3)
    d = res["diversity"]
    assert d["hypotheses"] == 8 and d["unique"] == 1.0 and 0.0 < d["distinct1"] <= 1.0
    assert d["mbleu1"] == d["mbleu2"] == d["mbleu3"] == d["mbleu4"] == 0
