"""GPU: ensemble decoding ("Ensemble decoding"): one batched beam search over several captioning models.  Shapes of
tests/test_gpu_constrained_search.py: V = 83 (every kernel's tail), 9 images, max_gen_length = 9, temperatures [1.0, 0.7], beam 4.

The combine kernel is held to the project's bound (b), 1e-4 * max(1, max|reference|), against tests/ensemble_ref.py in float64; the
search to the CPU reference within the GPU-vs-CPU bound 1e-4 and to the plain search of one member within the batched-vs-loop bound
1e-5.  Every model seed below was chosen on the CPU with ensemble_ref / history_ref alone so that no pick and no final order of the
reference rests on a near-tie; the tests assert those margins again."""
import ctypes as C

import pytest
import torch

import ensemble_ref as ER
import history_ref as HR
import test_ensemble as TE
import test_gpu_constrained_search as TC

pytestmark = pytest.mark.gpu

V, S, TEMPS, K = TC.V, TC.S, TC.TEMPS, 4
MODES = ("arithmetic", "geometric")
WEIGHTS3 = [0.5, 0.3, 0.2]
#: test 4, three heterogeneous members at (0.5, 0.3, 0.2): ensemble_ref's margins (measured: seed 25 boundary 2.5e-3, final 1.5e-2; seed 34
#: boundary 1.3e-3, final 9.2e-4); the ensemble's captions differ from every member's own on 9 of 9 images for both
REF_SEEDS = {"arithmetic": 25, "geometric": 34}
#: test 5, members 0 and 1 of that construction at (0.6, 0.4), min_length 3, no_repeat_ngram 2, <UNK> (80) and the two commonest words of
#: the un-ruled ensemble result banned (measured: seed 24 boundary 1.4e-3, final 4.2e-4; seed 18 boundary 1.2e-3, final 7.9e-4)
RULED = {"arithmetic": dict(seed=24, banned=[24, 44, 80]), "geometric": dict(seed=18, banned=[18, 74, 80])}
#: tests 3 and 6, one member with one LSTM layer and one with two (member 0 / 1 of the construction, each with a seed of its own):
#: history_ref's margins of the member alone (measured: seed 40 boundary 1.1e-3, final 5.4e-4; seed 1056 boundary 2.1e-3, final 1.8e-2)
SOLO = [(40, 0), (1056, 1)]
#: test 7, two whole models (resnet18 encoders; the second with two LSTM layers and deep output) at (0.6, 0.4): ensemble_ref's margins on the
#: annotations the encoders produce, which only a GPU gives (measured there: seed 6 boundary 8.6e-3, final 1.3e-2)
SURFACE_SEED = 6
_cache = {}


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _combine(lib, L, logits, weights, mode, T, out):
    M = len(logits)
    arr = (C.c_void_p * M)(*[z.data_ptr() for z in logits])
    wts = (C.c_float * M)(*weights)
    L.check(lib.sat_beam_ensemble_scores(arr, wts, M, L.ENSEMBLE_COMBINE[mode], logits[0].shape[0], logits[0].shape[1], T, L.ptr(out), L.stream_ptr()),
            "sat_beam_ensemble_scores")


@pytest.mark.parametrize("Vk", [83, 257, 1030])
def test_combine_kernel_against_float64(Vk):
    """1. 5 rows; M in {1, 2, 3, 8}, both modes, T in {1.0, 0.7}; with M >= 2 one member has weight 0 in a second run; row 2 of member 0
    spans +-60; at V = 83 and 257 the last member (and in a second layout the output) starts one float past a 16-byte boundary, at
    V = 1030 rows 0, 2 and 4 take the 16-byte path with a tail of two words.  Against ensemble_ref.combine in float64 within
    1e-4 * max(1, max|ref|); no NaN, no -inf; the guard row after the last row keeps its bits; two runs, same bits."""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    rows = 5
    g = torch.Generator().manual_seed(700 + Vk)
    worst = 0.0
    for M in (1, 2, 3, 8):
        host = [torch.randn(rows, Vk, generator=g) * 3.0 for _ in range(M)]
        host[0][2] = torch.where(torch.rand(Vk, generator=g) < 0.5, 60.0, -60.0)
        host[0][2, 5] = 60.0; host[0][2, 6] = -60.0
        raw = torch.rand(M, generator=g) + 0.1
        layouts = [(0, 0)] if Vk == 1030 else [(0, 0), (1, 0), (1, 1)]             # (offset of the last member, offset of the output) in floats
        for off_in, off_out in layouts:
            dev = []
            for i, z in enumerate(host):
                flat = torch.zeros(rows * Vk + 4, device="cuda")
                o = off_in if i == M - 1 else 0
                flat[o:o + rows * Vk] = z.reshape(-1).cuda()
                dev.append(flat[o:o + rows * Vk].view(rows, Vk))
            wsets = [(raw / raw.sum()).tolist()]
            if M >= 2:
                zero = raw.clone(); zero[M // 2] = 0.0
                wsets.append((zero / zero.sum()).tolist())
            for weights in wsets:
                for mode in MODES:
                    for T in (1.0, 0.7):
                        outs = []
                        for _ in range(2):
                            flat = torch.full(((rows + 1) * Vk + 4,), 123.0, device="cuda")
                            out = flat[off_out:off_out + (rows + 1) * Vk].view(rows + 1, Vk)
                            _combine(lib, L, dev, weights, mode, T, out)
                            outs.append(out)
                        torch.cuda.synchronize()
                        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
                        got = outs[0].cpu()
                        assert bool((got[rows] == 123.0).all()), "the guard row was written"
                        got = got[:rows].double()
                        assert bool(torch.isfinite(got).all()), (M, mode, T)
                        w32 = [float(torch.tensor(w, dtype=torch.float32)) for w in weights]
                        want = ER.combine(host, w32, mode, float(torch.tensor(T, dtype=torch.float32)))
                        bound = 1e-4 * max(1.0, float(want.abs().max()))
                        err = float((got - want).abs().max())
                        worst = max(worst, err / bound)
                        assert err <= bound, (M, mode, T, off_in, off_out, err, bound)
    print("V=%d: worst error / bound %.4f" % (Vk, worst))


# ------------------------------------------------------------------------------------------------ the search
def _gpu_member(seed, index):
    """member ``index`` of the heterogeneous construction built after ``torch.manual_seed(seed)``: (decoder on the GPU, hparams,
    annotations on the GPU, (h, w), what ensemble_ref takes); built once"""
    key = ("member", seed, index)
    if key not in _cache:
        over, hw = TE.HETERO[index]
        dec, hp, ann = TE.build_member(seed, over, hw, 55 + index)
        ref = TE.reference_member(dec, hp, ann, hw)
        _cache[key] = (dec.cuda().eval(), hp, ann.cuda().contiguous(), hw, ref)
    return _cache[key]


def _hetero(seed, count=3):
    return [_gpu_member(seed + 1000 * i, i) for i in range(count)]


def _ensemble(members, weights, mode):
    from sat_amd.ensemble import Ensemble
    return Ensemble([m[0] for m in members], weights, mode), [m[2] for m in members], members[0][3]


def _margins(m):
    return min(x for x in m["boundary"] if x is not None), min(g for img in m["final"] for g in img)


def _as_maps(res, hw):
    return res[0], res[1], [[a.reshape(-1, *hw) for a in al] for al in res[2]], res[3]


def _raw_ensemble(members, weights, mode, con=None, hist=None):
    """sat_beam_search_ensemble on zeroed buffers, as TC._raw calls its neighbours; members = [(decoder, hparams, annotations)]"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    B = members[0][2].shape[0]
    ens = L.BeamEnsemble(members=len(members), combine=L.ENSEMBLE_COMBINE[mode])
    keep = []
    for i, (dec, hp, ann) in enumerate(members):
        _, Lc, D = ann.shape
        dims = Dk.decoder_dims(B, K, 2, Lc, D, 16, 24, int(hp.decoder_dim), V, 0, hp.deep_output, dec.pad_idx, 0, layers=int(hp.decoder_layers))
        w, tens = dec._params_struct()
        keep += [dims, w, tens]
        ens.dims[i], ens.params[i], ens.ann[i], ens.weight[i] = C.pointer(dims), C.pointer(w), ann.data_ptr(), weights[i]
    Lc = members[0][2].shape[1]
    i32 = dict(dtype=torch.int32, device="cuda"); f32 = dict(dtype=torch.float32, device="cuda")
    o = dict(tok_in=torch.zeros(S + 2, B, K, **i32), prev_row=torch.zeros(S + 2, B, K, **i32), alpha_hist=torch.zeros(S + 1, B, K, Lc, **f32),
             fin_count=torch.zeros(B, **i32), fin_step=torch.zeros(B, K, **i32), fin_row=torch.zeros(B, K, **i32), fin_score=torch.zeros(B, K, **f32),
             fin_mean=torch.zeros(B, K, **f32))
    tarr = (C.c_float * len(TEMPS))(*TEMPS)
    ids = (C.c_int32 * 4)(*[int(members[0][1].vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    outs = [L.ptr(o[k]) for k in ("tok_in", "prev_row", "alpha_hist", "fin_count", "fin_step", "fin_row", "fin_score", "fin_mean")]
    nbytes = lib.sat_beam_search_ensemble_workspace_bytes(C.byref(ens), K, S)
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    L.check(lib.sat_beam_search_ensemble(C.byref(ens), K, S, tarr, len(TEMPS), ids, C.byref(con) if con is not None else None,
                                         C.byref(hist) if hist is not None else None, *outs, L.ptr(ws), nbytes, L.stream_ptr()), "sat_beam_search_ensemble")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("layers", [1, 2])
def test_one_member_is_the_plain_search(layers):
    """2. M = 1 through sat_beam_search_ensemble against sat_beam_search_sampled: the back-trace and the attention maps equal, the scores
    within 1e-5 relative (the combined logits of one member are its log-softmax, normalised once more)"""
    dec, hp, ann = TC._setup(layers, seed=TC.ORACLE_SEEDS[layers])
    want = TC._raw(dec, hp, ann, K, "sampled")
    assert int(want["fin_count"].min()) >= 1
    for mode in MODES:
        got = _raw_ensemble([(dec, hp, ann)], [1.0], mode)
        for k in ("tok_in", "prev_row", "fin_count", "fin_step", "fin_row", "alpha_hist"):
            assert torch.equal(got[k], want[k]), (mode, k)
        for k in ("fin_score", "fin_mean"):
            assert bool(((got[k] - want[k]).abs() <= 1e-5 * want[k].abs().clamp_min(1.0)).all()), (mode, k)


def _solo(which, precision="fp32"):
    """the plain batched search of one SOLO member, computed once per precision and left unchanged"""
    key = ("solo", which, precision)
    if key not in _cache:
        dec, _, ann, hw, _ = _gpu_member(*SOLO[which])
        dec.sat_precision = precision
        try:
            _cache[key] = dec.beam_decode_batched(ann, hw, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True)
        finally:
            dec.sat_precision = "fp32"
    return _cache[key]


def test_solo_members_are_margin_safe():
    """the seeds of tests 3 and 6: history_ref's margins of each member alone, and the GPU search against it (1e-4)"""
    for which in (0, 1):
        dec, hp, ann, hw, ref = _gpu_member(*SOLO[which])
        m = {}
        with torch.no_grad():
            want = HR.beam_search(*ref, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True, margins=m)
        b, f = _margins(m)
        print("member %d alone: boundary %.2e final %.2e" % (which, b, f))
        assert b >= 1e-3 and f >= 2e-4
        TC._close(_as_maps(want, hw), _solo(which), 1e-4)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("which", [0, 1])
def test_the_same_member_twice_is_that_member(which, precision):
    """3. (0.5, 0.5) of one model with itself, both modes, both precisions: captions and list order of the plain search at that
    precision, scores within 1e-5 (a second member's state gathered or fed wrongly would show here)"""
    m = _gpu_member(*SOLO[which])
    want = _solo(which, precision)
    m[0].sat_precision = precision
    try:
        for mode in MODES:
            ens, anns, hw = _ensemble([m, m], [0.5, 0.5], mode)
            got = ens.beam_decode_batched(anns, hw, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True)
            TC._close(want, got, 1e-5)
    finally:
        m[0].sat_precision = "fp32"


@pytest.mark.parametrize("mode", MODES)
def test_heterogeneous_members_against_the_cpu_reference(mode):
    """4. three members (1 layer, D 32, L 12 | 2 layers, D 48, L 6 | 1 layer, deep output, decoder_dim 56) at (0.5, 0.3, 0.2) against
    ensemble_ref.beam_search: captions and list order identical, scores, perplexities and member 0's maps within 1e-4; the reference's
    margins hold, and the ensemble decodes something none of its members decodes alone"""
    members = _hetero(REF_SEEDS[mode])
    kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True)
    m = {}
    with torch.no_grad():
        want = ER.beam_search([x[4] for x in members], WEIGHTS3, mode, margins=m, **kw)
    b, f = _margins(m)
    print("%s seed %d: boundary %.2e final %.2e" % (mode, REF_SEEDS[mode], b, f))
    assert b >= 1e-3 and f >= 2e-4
    ens, anns, hw = _ensemble(members, WEIGHTS3, mode)
    got = ens.beam_decode_batched(anns, hw, **kw)
    TC._close(_as_maps(want, hw), got, 1e-4)
    for dec, _, ann, hw_i, _ in members:
        alone = dec.beam_decode_batched(ann, hw_i, **kw)
        assert sum(a != g for a, g in zip(alone[0], got[0])) >= 1


@pytest.mark.parametrize("mode", MODES)
def test_rules_against_the_cpu_reference(mode):
    """5. two members at (0.6, 0.4) with banned ids (<UNK> among them), min_length 3 and no_repeat_ngram 2 against ensemble_ref"""
    case = RULED[mode]
    members = _hetero(case["seed"], 2)
    hp = members[0][1]
    unk = int(hp.vocab_stoi["<UNK>"])
    assert unk in case["banned"]
    kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True, min_length=3, no_repeat_ngram=2)
    m = {}
    with torch.no_grad():
        want = ER.beam_search([x[4] for x in members], [0.6, 0.4], mode, margins=m, banned=case["banned"], **kw)
    b, f = _margins(m)
    print("%s seed %d: boundary %.2e final %.2e" % (mode, case["seed"], b, f))
    assert b >= 1e-3 and f >= 2e-4
    ens, anns, hw = _ensemble(members, [0.6, 0.4], mode)
    got = ens.beam_decode_batched(anns, hw, banned=[t for t in case["banned"] if t != unk], no_unk=True, **kw)
    TC._close(_as_maps(want, hw), got, 1e-4)
    caps = [c for img in got[0] for c in img]
    assert not any(t in case["banned"] for c in caps for t in c)
    assert not any(HR.repeats_ngram(c, 2) for c in caps) and min(len(c) for c in caps) >= 3
    plain = ens.beam_decode_batched(anns, hw, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True)
    assert plain[0] != got[0]                               # the rules bite


@pytest.mark.parametrize("mode", MODES)
def test_a_weight_of_one_is_that_member_alone(mode):
    """6. weights (1, 0) and (0, 1): the weighted member's own captions, scores within 1e-5; alpha_hist holds member 0's maps either
    way (under (0, 1) they are member 0 attending along member 1's captions): finite, and every live row sums to 1"""
    members = [_gpu_member(*SOLO[0]), _gpu_member(*SOLO[1])]
    assert int(members[0][1].vocab_stoi["<PAD>"]) == 0     # a live row never holds token 0, a dead one always does
    for weights, which in (([1.0, 0.0], 0), ([0.0, 1.0], 1)):
        ens, anns, hw = _ensemble(members, weights, mode)
        got = ens.beam_decode_batched(anns, hw, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True)
        want = _solo(which)
        assert got[0] == want[0]
        for i in (1, 3):
            for u, v in zip(TC._flat(got[i]), TC._flat(want[i])):
                assert abs(u - v) <= 1e-5 * max(1.0, abs(v)), (weights, i, u, v)
        if which == 0:
            TC._close(want, got, 1e-5)
        o = ens._beam_search_device(anns, K, S, TEMPS, "beam", 3, None, None, None, None, False)
        alpha, live = o["alpha_hist"], o["tok_in"][:S + 1] != 0
        assert alpha.shape == (S + 1, 9, K, hw[0] * hw[1]) and bool(torch.isfinite(alpha).all()) and bool(live[0].all())
        sums = alpha.sum(-1)[live]
        assert float((sums - 1.0).abs().max()) <= 1e-5
        assert all(a.shape[1:] == hw for maps in got[2] for a in maps)


# ------------------------------------------------------------------------------------------------ 7. the surface
def _models():
    """two whole SAT models over one vocabulary (the second: two LSTM layers, deep output), a batch of images and its references"""
    if "models" not in _cache:
        import sat_amd  # noqa: F401
        from sat_amd import model as M
        from oracle import prng, sat_oracle as O
        over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40,
                    val_beamk=3, val_max_len=7)
        torch.manual_seed(SURFACE_SEED)
        m0 = M.SAT(**vars(O.default_hparams(**over))).cuda()
        torch.manual_seed(SURFACE_SEED + 1000)
        m1 = M.SAT(**vars(O.default_hparams(**dict(over, decoder_layers=2, deep_output=True)))).cuda()
        img = torch.from_numpy(prng.uniform((4, 3, 64, 64), 41, 0.0, 1.0)).cuda()
        caps, lengths = prng.captions(4, 3, 9, 60, 42, min_len=3)
        _cache["models"] = (m0, m1, img, torch.from_numpy(caps).cuda(), torch.from_numpy(lengths))
    return _cache["models"]


def test_surface_caption_in_the_reference_order():
    """7. Ensemble.caption with "LN" and return_all against ensemble_ref on the annotations the two encoders produced: captions and list
    order identical, values within 1e-4; the reference's margins are asserted"""
    from sat_amd.ensemble import Ensemble
    m0, m1, img, _, _ = _models()
    ens = Ensemble([m0, m1], [0.6, 0.4], "arithmetic")
    kw = dict(beamk=3, max_gen_length=7, temperature=TEMPS, rescore_method="LN", return_all=True)
    got = ens.caption(img, **kw)
    anns, hw = ens.encode(img)
    refs = []
    for m, ann in zip((m0, m1), anns):
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if not k.startswith("encoder.")}
        refs.append((sd, m.hp, ann.detach().cpu().reshape(ann.shape[0], hw[0], hw[1], ann.shape[2]).permute(0, 3, 1, 2).contiguous()))
    mg = {}
    with torch.no_grad():
        want = ER.beam_search(refs, [0.6, 0.4], "arithmetic", margins=mg, **kw)
    b, f = _margins(mg)
    print("surface seed %d: boundary %.2e final %.2e" % (SURFACE_SEED, b, f))
    assert b >= 1e-3 and f >= 2e-4
    TC._close(_as_maps(want, hw), got, 1e-4)
    best = ens.caption(img, **dict(kw, return_all=False))
    assert best[0] == [c[0] for c in got[0]] and best[1] == [s[0] for s in got[1]]
    assert all(len(c) == 3 for c in got[0]) and all(s == sorted(s, reverse=True) for s in got[1])


def test_surface_mbr_and_evaluation():
    """7. rescore_method="MBR" returns utilities; val_batch_stats(...).metrics() against score_captions on caption(...): bleu / gleu
    exactly, cosine within max(2 e_torch, 1e-6) of the float64 value, perplexity 1e-6 relative (the rule of the single-model pair);
    evaluate and random_search take the ensemble"""
    from sat_amd import evaluation as E
    from sat_amd.ensemble import Ensemble
    m0, m1, img, caps, lengths = _models()
    ens = Ensemble([m0, m1], combine="geometric")
    rc = E.ReferenceCorpus(60).add(caps, lengths).check()
    kw = dict(beamk=3, max_gen_length=7, temperature=1.0)
    plain = ens.caption(img, rescore_method=None, return_all=True, **kw)
    got = ens.caption(img, rescore_method="MBR", mbr_corpus=rc, return_all=True, **kw)
    assert [sorted(c) for c in got[0]] == [sorted(c) for c in plain[0]]       # the same hypotheses, reranked
    assert all(s == sorted(s, reverse=True) and all(u >= 0.0 for u in s) for s in got[1])
    kw = dict(kw, rescore_method="LN", rescore_reward=0.7, no_unk=True, min_length=2)
    captions, _, _, ppl = ens.caption(img, return_all=False, **kw)
    want = ens.score_captions(captions, caps, lengths, ppl)
    assert want == ens.val_batch((img, caps, lengths), **kw)
    stats = ens.val_batch_stats((img, caps, lengths), **kw).metrics()
    assert set(stats) == set(want)
    for k in ("bleu1", "bleu2", "bleu3", "bleu4", "gleu"):
        assert stats[k] == want[k], (k, stats[k], want[k])
    E64 = m0.embedding.weight.detach().cpu().double()
    c64 = []
    for i, h in enumerate(captions):
        cv = E64[torch.as_tensor(h, dtype=torch.long)].mean(0)
        rvs = [E64[caps[i][j][1:int(l)].cpu()].mean(0) for j, l in enumerate(lengths[i])]
        c64.append(max(float(((rv / rv.norm().clamp_min(1e-8)) * (cv / cv.norm().clamp_min(1e-8))).sum()) for rv in rvs))
    c64 = sum(c64) / len(c64)
    e_kernel, e_torch = abs(stats["cosine_similarity"] - c64), abs(want["cosine_similarity"] - c64)
    print("cosine: e_kernel %.3e  e_torch %.3e" % (e_kernel, e_torch))
    assert e_kernel <= max(2 * e_torch, 1e-6)
    assert abs(stats["perplexity"] - want["perplexity"]) <= 1e-6 * abs(want["perplexity"])
    tok, ln, sc, pp = ens.caption_tokens(img, **kw)
    assert [tok[i, :int(ln[i])].tolist() for i in range(4)] == captions
    res = E.evaluate(ens, [(img, caps, lengths)] * 2, **kw)
    assert res["batches"] == 2 and res["images"] == 8 and set(res["batch_mean"]) == set(res["corpus"]) >= set(want)
    for k in ("bleu1", "bleu4", "gleu"):
        assert abs(res["batch_mean"][k] - want[k]) <= 1e-12 and abs(res["corpus"][k] - want[k]) <= 1e-12
    space = dict(E.NOTEBOOK_SPACE, sample_methods=["beam"], decoder_noises=[0.0], beamks=[2, 3], max_gen_length=7)
    rows = E.random_search(ens, [(img, caps, lengths)], trials=2, space=space, seed=3, max_batches=1)
    assert len(rows) == 2 and all(r["sample_method"] == "beam" and "bleu4" in r for r in rows)
