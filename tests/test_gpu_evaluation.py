"""GPU: the on-device evaluation path (csrc/caption_score.hip, sat_amd/evaluation.py) against the host path it shadows:
sat_caption_stats bit-equal to the host restatement, sat_beam_select against beam_decode_batched's back-trace, the cosine against a
float64 recomputation under the "no worse than twice the fp32 emulation" rule, val_batch_stats / evaluate against val_batch and the
corpus functions, and the whole batch under stream capture."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import caption_stats_ref as R  # noqa: E402
from test_oracle_golden import sd_from  # noqa: E402


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def test_caption_stats_bit_equal_to_the_host_restatement(golden_dir):
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    corpora = dict(R.random_corpora()); corpora.update(R.g10_corpora(golden_dir)); corpora.update(R.edge_corpora())
    assert {"hyp_shorter_than_n", "hyp_empty", "repeat_once_and_twice", "two_refs_equally_close", "equal_gleu_ratio", "at_the_limits"} <= set(corpora)
    lib = L.lib()
    for name, (refs, caps) in corpora.items():
        lim = name == "at_the_limits"
        packed = R.pack(refs, caps, width=L.CAPTION_MAX_LEN if lim else None, T=L.CAPTION_MAX_LEN if lim else None)
        if lim:
            assert packed[0].shape[1] == L.CAPTION_MAX_LEN and packed[2].shape[1:] == (L.CAPTION_MAX_REFS, L.CAPTION_MAX_LEN)
            assert int(packed[1].max()) == L.CAPTION_MAX_LEN and int(packed[3].max()) == L.CAPTION_MAX_LEN
        tok, ln, rf, rl = _dev(*packed)
        B, W = tok.shape
        stats = torch.full((B, 12), -7, dtype=torch.int32, device="cuda")
        L.check(lib.sat_caption_stats(L.ptr(tok), L.ptr(ln), W, L.ptr(rf), L.ptr(rl), B, rf.shape[1], rf.shape[2], L.ptr(stats), L.stream_ptr()), "sat_caption_stats")
        got, want = stats.cpu().tolist(), R.corpus_stats(refs, caps)
        for b in range(B):
            assert got[b] == want[b], (name, b, got[b], want[b], caps[b], refs[b])


def _g7_decoder(golden_dir):
    from sat_amd import model as M
    from oracle import sat_oracle as O
    g = np.load(os.path.join(golden_dir, "g7_beam.npz"))
    sd = sd_from(g)
    V, m = sd["embedding.weight"].shape
    hp = O.default_hparams(vocab_size=V, embed_dim=m, decoder_dim=sd["lstm.weight_hh_l0"].shape[1],
                           encoder_dim=sd["attention.encoder_att.weight"].shape[1], attention_dim=sd["attention.encoder_att.weight"].shape[0])
    dec = M.SATDecoder(hp).cuda().eval()
    dec.load_decoder_state(sd)
    ann = torch.tensor(g["ann"])
    B, D, Hh, Ww = ann.shape
    return dec, ann.permute(0, 2, 3, 1).reshape(B, Hh * Ww, D).contiguous().cuda(), (Hh, Ww)


def _random_decoder():
    from sat_amd import model as M
    from oracle import prng, sat_oracle as O
    hp = O.default_hparams(vocab_size=83, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40, decoder_layers=2)
    torch.manual_seed(5)
    dec = M.SATDecoder(hp).cuda().eval()
    return dec, torch.from_numpy(prng.uniform((9, 12, 32), 55, 0.0, 1.0)).cuda(), (3, 4)


@pytest.mark.parametrize("which", ["g7", "random_two_layers"])
def test_beam_select_equals_the_host_back_trace(golden_dir, which):
    """every rescoring method, beams 1 / 3 / 5, a length cut that ends hypotheses early and one that does not: the tokens, the
    rescored value (bit for bit) and the attention maps of beam_decode_batched(return_all=False)"""
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    dec, ann, hw = _g7_decoder(golden_dir) if which == "g7" else _random_decoder()
    PAD = dec.pad_idx
    reward = 0.7                                   # not an fp32 number: the kernel must round it as torch does
    cut = False
    for rm in (None, "LN", "WR", "BAR"):
        for beamk in (1, 3, 5):
            for mgl in (3, 14):
                kw = dict(beamk=beamk, max_gen_length=mgl, temperature=[1.0, 0.8])
                caps, scores, alphas, ppl = dec.beam_decode_batched(ann, hw, rescore_method=rm, rescore_reward=reward, return_all=False, **kw)
                o = dec._beam_search_device(ann, beamk, mgl, [1.0, 0.8], "beam", 3, None, None, None, None, False)
                sel = E.select_hypotheses(o, PAD, rm, reward, with_alpha=True)
                toks, lens, sc, al = sel["tokens"].cpu(), sel["lengths"].cpu().tolist(), sel["scores"].cpu().tolist(), sel["alphas"].cpu()
                assert toks.shape == (ann.shape[0], mgl + 1) and al.shape == (ann.shape[0], mgl, ann.shape[1])
                fin_step = o["fin_step"].cpu()
                for b in range(ann.shape[0]):
                    n = lens[b]
                    assert toks[b, :n].tolist() == caps[b], (rm, beamk, mgl, b)
                    assert (toks[b, n:] == PAD).all() and sel["steps"][b].item() == n
                    assert sc[b] == scores[b], (rm, beamk, mgl, b, sc[b], scores[b])
                    assert torch.equal(al[b, :n].reshape(-1, *hw), alphas[b]) and not al[b, n:].any()
                    ppl_d = float(torch.exp(-sel["raw"][b] / sel["steps"][b].float()))
                    assert abs(ppl_d - ppl[b]) <= 1e-6 * ppl[b]
                if mgl == 3:
                    fc = o["fin_count"].cpu().tolist()
                    cut = cut or any(bool((fin_step[b, :fc[b]] == mgl).any()) for b in range(ann.shape[0]))
    assert cut, "no hypothesis ended by the length cut"
    # sampled search: the same seed gives the same captions on both paths
    for seed in (11, 12):
        kw = dict(beamk=4, max_gen_length=9, temperature=1.0, sample_method="multinomial", decoder_noise=0.2)
        caps, scores, _, _ = dec.beam_decode_batched(ann, hw, rescore_method="LN", return_all=False, seed=seed, **kw)
        o = dec._beam_search_device(ann, 4, 9, 1.0, "multinomial", 3, 0.2, seed, None, None, False)
        sel = E.select_hypotheses(o, PAD, "LN")
        assert sel["alphas"] is None
        lens = sel["lengths"].cpu().tolist()
        assert [sel["tokens"][b, :lens[b]].tolist() for b in range(ann.shape[0])] == caps and sel["scores"].cpu().tolist() == scores


def _cos64(E64, captions, caps, lengths):
    """best cosine per image in float64 (F.cosine_similarity's definition, eps = 1e-8)"""
    out = []
    for i, h in enumerate(captions):
        cv = E64[torch.as_tensor(h, dtype=torch.long)].mean(0)
        best = []
        for j, l in enumerate(lengths[i]):
            rv = E64[torch.as_tensor(caps[i][j][1:l], dtype=torch.long)].mean(0)
            best.append(float(((rv / rv.norm().clamp_min(1e-8)) * (cv / cv.norm().clamp_min(1e-8))).sum()))
        out.append(max(best))
    return out


def _cos_torch_loop(E, captions, enc, lens):
    """the fp32 loop of SAT.score_captions (model.py:660-673), per image"""
    dev = E.device
    cossims = torch.zeros(enc.shape[0], dtype=torch.float, device=dev)
    for i in range(enc.shape[0]):
        cv = E[torch.as_tensor(captions[i], dtype=torch.long, device=dev)].mean(0).unsqueeze(0)
        rvs = torch.zeros(enc.shape[1], dtype=torch.float, device=dev)
        for j, l in enumerate(lens[i]):
            rv = E[enc[i][j][1:l]].mean(0).unsqueeze(0)
            rvs[j] = F.cosine_similarity(rv, cv)
        cossims[i] = rvs.max()
    return cossims


@pytest.mark.parametrize("V,m,B,Rn,T,W", [(60, 24, 16, 3, 9, 8), (6400, 256, 32, 5, 22, 33), (500, 300, 8, 8, 64, 65), (97, 2048, 4, 2, 12, 12)])
def test_caption_cosine_no_worse_than_twice_the_torch_loop(V, m, B, Rn, T, W):
    """|kernel - float64| <= max(2 |score_captions' fp32 loop - float64|, 1e-6), maxima over the images of a case"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    rs = np.random.RandomState(V + m)
    Ew = torch.from_numpy(rs.standard_normal((V, m)).astype(np.float32) + 0.3).cuda()
    lens = rs.randint(2, T + 1, size=(B, Rn))                       # c[1:l]: 1 .. T-1 tokens
    enc = rs.randint(0, V, size=(B, Rn, T))
    hl = rs.randint(1, W + 1, size=B)
    captions = [rs.randint(0, V, size=n).tolist() for n in hl]
    tok = np.zeros((B, W), np.int32)
    for b, h in enumerate(captions):
        tok[b, :len(h)] = h
    tok_d, hl_d, enc_d, lens_d = _dev(tok, hl.astype(np.int32), enc.astype(np.int32), lens.astype(np.int32))
    best = torch.empty(B, dtype=torch.float32, device="cuda")
    L.check(L.lib().sat_caption_cosine(L.ptr(tok_d), L.ptr(hl_d), W, L.ptr(enc_d), L.ptr(lens_d), B, Rn, T, L.ptr(Ew), V, m, L.ptr(best), L.stream_ptr()),
            "sat_caption_cosine")
    want = torch.tensor(_cos64(Ew.cpu().double(), captions, enc.tolist(), lens.tolist()), dtype=torch.float64)
    loop = _cos_torch_loop(Ew, captions, torch.from_numpy(enc).cuda(), lens.tolist())
    e_kernel = float((best.cpu().double() - want).abs().max())
    e_torch = float((loop.cpu().double() - want).abs().max())
    print("cosine V=%d m=%d: e_kernel %.3e  e_torch %.3e  ratio %.2f" % (V, m, e_kernel, e_torch, e_kernel / max(e_torch, 1e-30)))
    assert e_kernel <= max(2 * e_torch, 1e-6)


def _val_model():
    """the model and the batch maker of test_validation_step_scores_generated_captions"""
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


def _check_against_val_batch(got, want, cos64, label):
    """bleu1-4 / gleu exactly; cosine within max(2 e_torch, 1e-6) of the float64 value; perplexity 1e-6 relative"""
    for k in ("bleu1", "bleu2", "bleu3", "bleu4", "gleu"):
        assert got[k] == want[k], (label, k, got[k], want[k])
    e_kernel, e_torch = abs(got["cosine_similarity"] - cos64), abs(want["cosine_similarity"] - cos64)
    print("%s cosine: e_kernel %.3e  e_torch %.3e" % (label, e_kernel, e_torch))
    assert e_kernel <= max(2 * e_torch, 1e-6), (label, got["cosine_similarity"], want["cosine_similarity"], cos64)
    assert abs(got["perplexity"] - want["perplexity"]) <= 1e-6 * abs(want["perplexity"]), (label, got["perplexity"], want["perplexity"])


@pytest.mark.parametrize("rm", ["LN", "BAR"])
def test_val_batch_stats_agrees_with_val_batch(rm):
    import sat_amd  # noqa: F401
    model, batch = _val_model()
    b = batch(41)
    kw = dict(beamk=3, max_gen_length=7, temperature=1.0, rescore_method=rm, rescore_reward=0.7)
    want = model.val_batch(b, **kw)
    got = model.val_batch_stats(b, **kw).metrics()
    assert set(got) == set(want) == {"bleu1", "bleu2", "bleu3", "bleu4", "cosine_similarity", "gleu", "perplexity"}
    captions = model.caption(b[0], return_all=False, **kw)[0]
    c64 = _cos64(model.embedding.weight.detach().cpu().double(), captions, b[1].tolist(), b[2].tolist())
    _check_against_val_batch(got, want, sum(c64) / len(c64), rm)


def test_evaluate_batch_mean_and_corpus_over_three_batches():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, metrics
    model, batch = _val_model()
    loader = [batch(s) for s in (41, 51, 61)]
    kw = dict(beamk=3, max_gen_length=7, temperature=1.0, rescore_method="LN")
    res = E.evaluate(model, loader, **kw)
    assert res["batches"] == 3 and res["images"] == 12
    per = [model.val_batch(b, **kw) for b in loader]
    mean = {k: sum(p[k] for p in per) / 3 for k in per[0]}
    E64 = model.embedding.weight.detach().cpu().double()
    captions, refs, c64 = [], [], []
    for b in loader:
        caps_b = model.caption(b[0], return_all=False, **kw)[0]
        captions += caps_b
        refs += [[c[1:l] for c, l in zip(r, b[2][i].tolist())] for i, r in enumerate(b[1].tolist())]
        one = _cos64(E64, caps_b, b[1].tolist(), b[2].tolist())
        c64.append(sum(one) / len(one))
    _check_against_val_batch(res["batch_mean"], mean, sum(c64) / 3, "batch_mean")
    for k, w in E.BLEU_WEIGHTS.items():
        assert res["corpus"][k] == metrics.corpus_bleu(refs, captions, weights=w), k
    assert res["corpus"]["gleu"] == metrics.corpus_gleu(refs, captions)
    total = model.val_batch_stats(loader[0], **kw) + model.val_batch_stats(loader[1], **kw) + model.val_batch_stats(loader[2], **kw)
    assert total.metrics() == res["corpus"]


def test_batch_scoring_runs_under_stream_capture():
    """caption_tokens + the statistics of one batch captured into a graph and replayed: equal to the eager call, also for new
    pictures in the static input.  A hidden synchronisation or host read would fail the capture."""
    import sat_amd  # noqa: F401
    model, batch = _val_model()
    kw = dict(beamk=3, max_gen_length=7, temperature=1.0, rescore_method="BAR", rescore_reward=0.7)
    b1, b2 = batch(41), batch(51)
    static = [b1[0].clone(), b1[1].clone(), b1[2].cuda()]
    eager = {}
    for name, b in (("b1", b1), ("b2", b2)):
        dev_b = (b[0], b[1], b[2].cuda())
        eager[name] = (model.val_batch_stats(dev_b, **kw).vector().clone(), [t.clone() for t in model.caption_tokens(b[0], **kw)])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vec = model.val_batch_stats(tuple(static), **kw).vector()
        toks = model.caption_tokens(static[0], **kw)
    for name, b in (("b1", b1), ("b2", b2), ("b1", b1)):
        static[0].copy_(b[0]); static[1].copy_(b[1]); static[2].copy_(b[2].cuda())
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(vec, eager[name][0]), name
        for u, v in zip(toks, eager[name][1]):
            assert torch.equal(u, v), name
    assert not torch.equal(eager["b1"][0], eager["b2"][0])
