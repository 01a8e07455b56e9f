"""GPU: consensus (minimum-Bayes-risk) reranking of the finished beam ("Consensus reranking"): sat_beam_hypotheses,
sat_caption_mbr and sat_beam_select_at against their host specification (sat_amd/metrics.py: consensus_utilities) and the host
back-trace, then the three chained behind the batched search.

Bound per utility (mbr_cases.bound): wc * 1e-9 + wr * 1e-12 + 1e-12 |want|.  The first two are the project's tolerances for CIDEr-D and
ROUGE-L (tests/test_gpu_consensus.py), and a weighted mean cannot exceed its terms' error; the relative term covers the fp64 exp of the
weights q_j, a few ulp, at three orders of margin.  Winners are compared exactly wherever the host's best and second-best utility are
>= 1e-6 apart, far above the bound; mbr_cases.BEAM_SEED was chosen on the CPU with metrics.py alone so that at least 3/4 of the
non-degenerate images are such (asserted below from the host values only), elsewhere the device's winner must be within 2 bounds of
the host's best, and an exact tie must go to index 0."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import consensus_cases  # noqa: E402
import mbr_cases as MC  # noqa: E402
import test_gpu_consensus as TG  # noqa: E402
import test_gpu_constrained_search as TC  # noqa: E402

SENTINEL, GUARD = -777, 64
_host = {}
_corpora = {}


def _metrics():
    import sat_amd  # noqa: F401
    from sat_amd import metrics
    return metrics


def _table(kind):
    """``(ReferenceCorpus, df, n_images)`` of the three tables, built once"""
    from sat_amd import evaluation as E
    if kind not in _corpora:
        refs = MC.corpus_refs()
        if kind == "one":
            refs = refs[:1]
        df = _metrics().document_frequency(refs)
        rc = TG.build(refs, 24, vocab=12, capacity=E._pow2_at_least(len(df) + 1) if kind == "crowded" else None).check()
        assert rc.to_dict() == df
        if kind == "crowded":
            assert len(df) < rc.capacity <= 2 * len(df)
        _corpora[kind] = (rc, df, len(refs))
    return _corpora[kind]


def _host_utilities(K, W, kind, reward, alpha):
    """metrics.consensus_utilities of every image of mbr_cases.beams(K, W): computed once, shared, left unchanged"""
    key = (K, W, "random" if kind == "crowded" else kind, reward, alpha)
    if key not in _host:
        m = _metrics()
        refs = MC.corpus_refs()[:1] if kind == "one" else MC.corpus_refs()
        df = m.document_frequency(refs)
        hyps, logps = MC.beams(K, W)
        _host[key] = [m.consensus_utilities(h, s, df, len(refs), reward, alpha) for h, s in zip(hyps, logps)]
    return _host[key]


def _device_beams(K, W):
    hyps, logps = MC.beams(K, W)
    return hyps, [torch.from_numpy(a).cuda() for a in MC.pack_beams(hyps, logps, K, W)]


# ----------------------------------------------------------------------------- 1. sat_beam_hypotheses
@pytest.mark.parametrize("S", [1, 9, 127])
@pytest.mark.parametrize("K", [1, 4, 32])
def test_beam_hypotheses_against_the_host_back_trace(K, S):
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    B, W, pad = 9, S + 1, 1
    t = MC.trace_tables(B, K, S, seed=100 * K + S)
    assert t["fin_count"].min() == 0 and t["fin_count"].max() == K and t["fin_step"][:, 0].max() > S
    d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    tok_buf = torch.full((GUARD + B * K * W + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    len_buf = torch.full((GUARD + B * K + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    L.check(L.lib().sat_beam_hypotheses(L.ptr(d["tok_in"]), L.ptr(d["prev_row"]), L.ptr(d["fin_count"]), L.ptr(d["fin_step"]), L.ptr(d["fin_row"]), B, K, S,
                                        pad, L.ptr(tok_buf[GUARD:]), L.ptr(len_buf[GUARD:]), L.stream_ptr()), "sat_beam_hypotheses")
    tok, ln = tok_buf.cpu().numpy(), len_buf.cpu().numpy()
    for buf, n in ((tok, B * K * W), (ln, B * K)):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all()
    tok, ln = tok[GUARD:GUARD + B * K * W].reshape(B, K, W), ln[GUARD:GUARD + B * K].reshape(B, K)
    for b in range(B):
        for f in range(K):
            want = MC.host_trace(t, b, f, S, K) if f < t["fin_count"][b] else []
            assert ln[b, f] == len(want), (b, f)
            assert tok[b, f].tolist() == want + [pad] * (W - len(want)), (b, f)
    # the wrapper on the same tables
    from sat_amd import evaluation as E
    ht, hl = E.finished_hypotheses(d, pad)
    assert np.array_equal(ht.cpu().numpy(), tok) and np.array_equal(hl.cpu().numpy(), ln)


# ----------------------------------------------------------------------------- 2. sat_caption_mbr
def _check_image(label, b, count, got_u, got_w, want, reward, kind):
    """utilities within the bound, unused slots 0.0; the winner is the first maximum of the device's own utilities (so an exact tie
    goes to index 0), equals the host's wherever the host is clear, and is within 2 bounds of the host's best elsewhere"""
    for f, w in enumerate(want):
        assert abs(got_u[f] - w) <= MC.bound(reward, w), (label, b, f, got_u[f], w)
    assert all(u == 0.0 for u in got_u[count:]), (label, b)
    if count == 0:
        assert got_w == 0, (label, b)
        return
    assert got_w == got_u.index(max(got_u[:count])), (label, b, got_w)
    if kind == "one" and reward[1] == 0.0:                              # log N = 0: every CIDEr weight and with it every utility is 0
        assert all(u == 0.0 for u in got_u) and got_w == 0, (label, b)
    top = sorted(want, reverse=True)
    if count >= 2 and top[0] - top[1] >= MC.GAP:
        assert got_w == want.index(top[0]), (label, b, got_w)
    else:
        assert want[got_w] >= top[0] - 2 * MC.bound(reward, top[0]), (label, b, got_w)


@pytest.mark.parametrize("kind", ["random", "one", "crowded"])
@pytest.mark.parametrize("K,W", MC.SHAPES)
def test_caption_mbr_against_the_host(K, W, kind):
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    rc, _, n_images = _table(kind)
    hyps, (tok, ln, cnt, lp) = _device_beams(K, W)
    assert sorted(set(len(h) for h in hyps)) == list(range(K + 1))
    assert {0, 1, W} <= {len(c) for h in hyps for c in h}
    # every setting on the roomy table; the one-image and the crowded table with one CIDEr-only and one mixed setting
    settings = MC.REWARDS if kind == "random" else [MC.REWARDS[0], MC.REWARDS[2]]
    for reward, alpha in settings:
        label = (K, W, kind, reward, alpha)
        util, win = E.consensus_utilities(tok, ln, cnt, lp if alpha else None, rc, reward, alpha)
        assert util.shape == (len(hyps), K) and util.dtype == torch.float64 and win.dtype == torch.int32
        again = E.consensus_utilities(tok, ln, cnt, lp, rc, reward, alpha)
        assert torch.equal(again[0].view(torch.int64), util.view(torch.int64)) and torch.equal(again[1], win)          # the same bits
        want = _host_utilities(K, W, kind, reward, alpha)
        got_u, got_w = util.cpu().tolist(), win.cpu().tolist()
        worst = max([abs(g - w) for gu, wu in zip(got_u, want) for g, w in zip(gu, wu)] or [0.0])
        print("K=%d W=%d %s reward=%s alpha=%g: worst |device - host| = %.3e" % (K, W, kind, reward, alpha, worst))
        for b, h in enumerate(hyps):
            _check_image(label, b, len(h), got_u[b], got_w[b], want[b], reward, kind)
        dup = K + 1                                                     # the identical hypotheses: with uniform votes an exact tie
        assert len(set(map(tuple, hyps[dup]))) == 1
        if alpha == 0.0:
            assert got_w[dup] == 0 and len(set(got_u[dup][:len(hyps[dup])])) == 1 and len(set(want[dup])) == 1
        if kind == "crowded":                                           # the same content gives the same bits, wherever the slots are
            roomy = E.consensus_utilities(tok, ln, cnt, lp, _table("random")[0], reward, alpha)
            assert torch.equal(roomy[0].view(torch.int64), util.view(torch.int64)) and torch.equal(roomy[1], win)


def test_enough_images_have_a_clear_winner_on_the_host():
    """the exact winner comparison above cannot pass by skipping: from the host values alone, at least 3/4 of the non-degenerate images
    (two hypotheses or more, a table of more than one image) keep best and second best >= 1e-6 apart, for every setting"""
    for reward, alpha in MC.REWARDS:
        clear = total = 0
        for K, W in MC.SHAPES:
            for want in _host_utilities(K, W, "random", reward, alpha):
                if len(want) >= 2:
                    top = sorted(want, reverse=True)
                    total += 1; clear += top[0] - top[1] >= MC.GAP
        print("reward=%s alpha=%g: %d of %d images clear" % (reward, alpha, clear, total))
        assert 4 * clear >= 3 * total, (reward, alpha, clear, total)


def test_worked_example_on_the_device():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    _, _, rf, rl = TG.pack(consensus_cases.REFS, consensus_cases.HYPS, T=8, W=8)
    rc = E.ReferenceCorpus(40).add(rf, rl).check()
    tok, ln, cnt, lp = [torch.from_numpy(a).cuda() for a in MC.pack_beams([MC.HYPS], [MC.LOGPS], 7, 6)]
    for reward, alpha, want, winner in MC.WORKED:
        util, win = E.consensus_utilities(tok, ln, cnt, lp, rc, reward, alpha)
        got = util[0].tolist()
        assert all(abs(g - w) <= MC.bound(reward, w) for g, w in zip(got, want)) and got[5:] == [0.0, 0.0], (reward, alpha, got)
        assert int(win[0]) == winner


# ----------------------------------------------------------------------------- 3. sat_beam_select_at
def _select_at(d, pick, pick_score, pad, with_alpha):
    from sat_amd import _lib as L
    S, (B, K), Lc = d["tok_in"].shape[0] - 2, d["tok_in"].shape[1:], d["alpha_hist"].shape[-1]
    i32 = dict(dtype=torch.int32, device="cuda"); f32 = dict(dtype=torch.float32, device="cuda")
    out = dict(tokens=torch.full((B, S + 1), SENTINEL, **i32), lengths=torch.empty(B, **i32), scores=torch.empty(B, **f32), raw=torch.empty(B, **f32),
               steps=torch.empty(B, **i32), alphas=torch.empty(B, S, Lc, **f32) if with_alpha else None)
    L.check(L.lib().sat_beam_select_at(L.ptr(d["tok_in"]), L.ptr(d["prev_row"]), L.ptr(d["fin_count"]), L.ptr(d["fin_step"]), L.ptr(d["fin_row"]),
                                       L.ptr(d["fin_score"]), L.ptr(d["alpha_hist"]) if with_alpha else None, L.ptr(pick), L.ptr(pick_score), B, K, S, Lc,
                                       pad, L.ptr(out["tokens"]), L.ptr(out["lengths"]), L.ptr(out["scores"]), L.ptr(out["raw"]), L.ptr(out["steps"]),
                                       L.ptr(out["alphas"]), L.stream_ptr()), "sat_beam_select_at")
    return out


@pytest.mark.parametrize("K,S", [(1, 1), (4, 9), (32, 127)])
def test_beam_select_at_reproduces_beam_select(K, S):
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    B, Lc, pad = 9, 5, 1
    t = MC.trace_tables(B, K, S, seed=7 * K + S)
    rs = np.random.RandomState(K + S)
    t["fin_mean"] = rs.uniform(0.0, 2.0, size=(B, K)).astype(np.float32)
    t["alpha_hist"] = rs.uniform(0.0, 1.0, size=(S + 1, B, K, Lc)).astype(np.float32)
    for b in range(B):                             # sat_beam_select divides by the step of a used slot: keep those in range
        for f in range(int(t["fin_count"][b])):
            t["fin_step"][b, f] = min(max(int(t["fin_step"][b, f]), 1), S)
    d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    count = t["fin_count"]
    for method in (None, "LN", "WR", "BAR"):
        ref = E.select_hypotheses(d, pad, method, 0.7, with_alpha=True)
        raw = ref["raw"].cpu().numpy()
        pick = np.zeros(B, np.int32)
        for b in range(B):                         # the raw scores of an image are all different: the winner is the slot that holds cap_raw
            if count[b]:
                hit = np.nonzero(t["fin_score"][b, :count[b]] == raw[b])[0]
                assert len(hit) == 1
                pick[b] = hit[0]
        got = _select_at(d, torch.from_numpy(pick).cuda(), None, pad, True)
        for k in ("tokens", "lengths", "raw", "steps", "alphas"):
            assert torch.equal(got[k], ref[k]), (method, k)
        assert torch.equal(got["scores"][torch.from_numpy(count > 0).cuda()], ref["raw"][torch.from_numpy(count > 0).cuda()])
    # pick_score given: the cast of the picked entry; out-of-range picks are clamped into the finished slots
    score = rs.uniform(-3.0, 3.0, size=(B, K))
    pick = np.array([(-3, K + 5, 0, K - 1, 10 ** 6, -10 ** 6, 1, 2, 3)[b] for b in range(B)], np.int32)
    got = _select_at(d, torch.from_numpy(pick).cuda(), torch.from_numpy(score).cuda(), pad, False)
    tok, ln, sc, rw = (got[k].cpu().numpy() for k in ("tokens", "lengths", "scores", "raw"))
    for b in range(B):
        p = int(np.clip(pick[b], 0, max(int(count[b]) - 1, 0)))
        want = MC.host_trace(t, b, p, S, K) if count[b] else []
        assert ln[b] == len(want) and tok[b].tolist() == want + [pad] * (S + 1 - len(want)), b
        assert sc[b] == np.float32(score[b, p]) and rw[b] == (t["fin_score"][b, p] if count[b] else 0.0), b


# ----------------------------------------------------------------------------- 4. end to end behind the batched search
#: model seeds chosen on the CPU with the float64 search restatement (oracle beam_search) and metrics.py: with them the consensus winner
#: differs from the raw-score winner on at least three images (every caption within 1e-6 of the best utility is another one) and the best
#: utility is non-zero on all nine, for both settings of E2E; the raw winners lead by >= 0.019 (asserted below on the device's own lists)
MBR_SEEDS = {1: 2, 2: 1}
E2E = [((1.0, 0.0), 0.0), ((0.5, 0.5), 1.0)]


def _e2e_corpus():
    """37 images x 5 references over the tiny models' 83 words"""
    if "e2e" not in _corpora:
        refs = consensus_cases.random_corpus(vocab=TC.V - 4, seed=11)[0]
        _corpora["e2e"] = (TG.build(refs, 24, vocab=TC.V).check(), _metrics().document_frequency(refs), len(refs))
    return _corpora["e2e"]


@pytest.mark.parametrize("layers", [1, 2])
def test_mbr_behind_the_batched_search(layers):
    from sat_amd import evaluation as E
    m = _metrics()
    dec, hp, ann = TC._setup(layers, seed=MBR_SEEDS[layers])
    rc, df, n_images = _e2e_corpus()
    kw = dict(beamk=4, max_gen_length=TC.S, temperature=TC.TEMPS)
    base = dec.beam_decode_batched(ann, TC.HW, rescore_method=None, return_all=True, **kw)
    ln_plain = dec.beam_decode_batched(ann, TC.HW, rescore_method="LN", return_all=True, **kw)
    for reward, alpha in E2E:
        mb = dict(mbr_corpus=rc, mbr_reward=reward, mbr_alpha=alpha)
        # the reference rules do not see the keywords
        TC._same(dec.beam_decode_batched(ann, TC.HW, rescore_method=None, return_all=True, **kw, **mb), base)
        TC._same(dec.beam_decode_batched(ann, TC.HW, rescore_method="LN", return_all=True, **kw, **mb), ln_plain)
        host = [m.consensus_utilities(caps, sc, df, n_images, reward, alpha) for caps, sc in zip(base[0], base[1])]
        got = dec.beam_decode_batched(ann, TC.HW, rescore_method="MBR", **kw, **mb)
        every = dec.beam_decode_batched(ann, TC.HW, rescore_method="MBR", return_all=True, **kw, **mb)
        o = dec._beam_search_device(ann, 4, TC.S, TC.TEMPS, "beam", 3, None, None, None, None, False)
        sel = E.select_hypotheses(o, dec.pad_idx, "MBR", **mb)
        dev_tok, dev_len, dev_sc = sel["tokens"].cpu().tolist(), sel["lengths"].cpu().tolist(), sel["scores"].cpu().tolist()
        differs = nonzero = 0
        for b in range(9):
            caps, u = base[0][b], host[b]
            # a caption cut at max_gen_length and one that said <END> there can share their words: a hypothesis is (words, perplexity)
            keys = [(tuple(c), p) for c, p in zip(caps, base[3][b])]
            assert len(set(keys)) == len(keys), b
            best = max(u)
            tol = 2 * MC.bound(reward, best)
            i = keys.index((tuple(got[0][b]), got[3][b]))               # perplexity stays exp(-raw / steps)
            assert u[i] >= best - tol, (b, u, i)
            assert abs(got[1][b] - u[i]) <= MC.bound(reward, u[i]), (b, got[1][b], u[i])
            assert dev_tok[b][:dev_len[b]] == got[0][b] and dev_tok[b][dev_len[b]:] == [dec.pad_idx] * (TC.S + 1 - dev_len[b]), b
            assert dev_sc[b] == np.float32(got[1][b]), b
            assert torch.equal(got[2][b], base[2][b][i]), b             # the maps of that caption
            differs += got[0][b] != caps[0]
            nonzero += best > 0.0
            # return_all: the same hypotheses, by utility
            order = [keys.index((tuple(c), p)) for c, p in zip(every[0][b], every[3][b])]
            assert sorted(order) == list(range(len(keys))) and order[0] == i, b
            assert all(u[order[k]] >= u[order[k + 1]] - tol for k in range(len(order) - 1)), (b, [u[k] for k in order])
            assert all(abs(s - u[k]) <= MC.bound(reward, u[k]) for s, k in zip(every[1][b], order)), b
            assert all(torch.equal(a, base[2][b][k]) for a, k in zip(every[2][b], order)), b
        print("layers=%d reward=%s alpha=%g: consensus differs from the raw winner on %d of 9 images, best utility non-zero on %d" % (layers, reward, alpha, differs, nonzero))
        assert differs >= 1 and 2 * nonzero >= 9


def test_mbr_refusals_come_before_any_launch():
    dec, hp, ann = TC._setup(1)
    rc, _, _ = _e2e_corpus()
    kw = dict(max_gen_length=TC.S, temperature=TC.TEMPS, rescore_method="MBR")
    for bad in (dict(beamk=4), dict(beamk=4, mbr_corpus=rc, mbr_reward=(0.0, 0.0)), dict(beamk=4, mbr_corpus=rc, mbr_alpha=-1.0),
                dict(beamk=4, mbr_corpus=rc, mbr_reward=(float("nan"), 1.0)), dict(beamk=33, mbr_corpus=rc)):
        with pytest.raises(ValueError):
            dec.beam_decode_batched(ann, TC.HW, **kw, **bad)
    with pytest.raises(ValueError, match="batched"):
        dec.beam_decode(ann, TC.HW, beamk=4, **kw)


# ----------------------------------------------------------------------------- 5. val_batch_stats / evaluate / random_search
def test_val_batch_stats_and_evaluate_with_mbr():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    model, batch = TG._val_model()
    loader = [batch(s) for s in (41, 51, 61)]
    rc = E.ReferenceCorpus(60)
    for b in loader:
        rc.add(b[1], b[2])
    rc.check()
    kw = dict(beamk=3, max_gen_length=7, temperature=1.0, rescore_method="MBR", mbr_reward=(0.5, 0.5), mbr_alpha=1.0)
    emb = model.embedding.weight.detach().contiguous()
    vectors = []
    for b in loader:
        tok, ln, sc, ppl = model.caption_tokens(b[0], mbr_corpus=rc, **kw)
        caps, scores, _, ppls = model.caption(b[0], mbr_corpus=rc, **kw)
        assert [t[:n] for t, n in zip(tok.tolist(), ln.tolist())] == caps and sc.tolist() == [float(np.float32(s)) for s in scores]
        assert all(abs(p - q) <= 1e-6 * abs(q) for p, q in zip(ppl.tolist(), ppls))
        refs, rl = b[1].to(torch.int32).contiguous(), b[2].to(device="cuda", dtype=torch.int32).contiguous()
        stats, best = E.caption_statistics(tok, ln, refs, rl, emb)
        got = model.val_batch_stats(b, mbr_corpus=rc, **kw)
        assert got.vector().shape == (14,) and got.images == 4
        assert torch.equal(got.counts, stats.sum(0, dtype=torch.int64)) and torch.equal(got.cosine_sum, best.sum(dtype=torch.float64))
        assert torch.equal(got.perplexity_sum, ppl.sum(dtype=torch.float64))
        fallback = model.val_batch_stats(b, corpus=rc, **kw)                                       # mbr_corpus=None falls back to corpus=
        assert fallback.vector().shape == (16,) and torch.equal(fallback.vector()[:14], got.vector())
        vectors.append(got.vector())
        with pytest.raises(ValueError, match="mbr_corpus"):
            model.val_batch_stats(b, **kw)
    res = E.evaluate(model, loader, mbr_corpus=rc, **kw)
    rows = torch.stack(vectors).cpu().tolist()
    per_batch = [E.metrics_from_vector(r, 4) for r in rows]
    assert res["images"] == 12 and res["batches"] == 3
    assert res["batch_mean"] == {k: sum(d[k] for d in per_batch) / 3 for k in E.METRIC_KEYS}
    total = [sum(int(r[c]) for r in rows) for c in range(12)] + [sum(r[c] for r in rows) for c in (12, 13)]
    assert res["corpus"] == E.metrics_from_vector(total, 12)
    space = dict(E.NOTEBOOK_SPACE, beamks=[3], rescore_methods=["MBR"], sample_methods=["beam"], max_gen_length=7)
    out = E.random_search(model, loader, trials=1, space=space, seed=3, max_batches=1, mbr_corpus=rc)
    assert out[0]["rescore_method"] == "MBR" and set(E.METRIC_KEYS) <= set(out[0])
    with pytest.raises(ValueError, match="MBR"):
        E.random_search(model, loader, trials=1, space=space, seed=3, max_batches=1)


def test_the_three_launches_run_under_stream_capture():
    """hypotheses -> utilities -> select_at captured into a graph and replayed: no hidden synchronisation, allocation or host read"""
    from sat_amd import evaluation as E
    dec, hp, ann = TC._setup(1, seed=MBR_SEEDS[1])
    rc, _, _ = _e2e_corpus()
    o = dec._beam_search_device(ann, 4, TC.S, TC.TEMPS, "beam", 3, None, None, None, None, False)
    mb = dict(mbr_corpus=rc, mbr_reward=(0.5, 0.5), mbr_alpha=1.0)
    eager = E.select_hypotheses(o, dec.pad_idx, "MBR", with_alpha=True, **mb)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = E.select_hypotheses(o, dec.pad_idx, "MBR", with_alpha=True, **mb)
    g.replay()
    torch.cuda.synchronize()
    for k in ("tokens", "lengths", "scores", "raw", "steps", "alphas", "winner"):
        assert torch.equal(out[k], eager[k]), k
    assert torch.equal(out["utilities"].view(torch.int64), eager["utilities"].view(torch.int64))
