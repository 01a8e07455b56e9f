"""GPU: required words of the batched caption search ("Required words").  Shapes, helpers and models of
tests/test_gpu_constrained_search.py: V = 83 (every kernel's tail), 9 images, L = 12, max_gen_length = 9, temperatures [1.0, 0.7], one and
two LSTM layers.

The selection kernel is checked bit for bit against the numpy restatement tests/required_ref.select, the search against
tests/required_ref.beam_search within the project's GPU-vs-CPU bound 1e-4, the search with the words off against
sat_beam_search_history bit for bit.  Every model seed below was chosen on the CPU with required_ref / history_ref alone so that no pick
and no final order of the reference rests on a near-tie; the tests assert those margins again."""
import ctypes as C

import numpy as np
import pytest
import torch

import history_ref as HR
import required_ref as RR
import test_gpu_constrained_search as TC
import test_gpu_search_history as TH
import test_required_search as TR

pytestmark = pytest.mark.gpu

V, S, HW, TEMPS = TC.V, TC.S, TC.HW, TC.TEMPS
#: test 3 (and 2, 4, 5, which reuse "k4_c2"): case -> {layers: seed}.  required_ref's search keeps >= 1e-3 at every selection (every bank's
#: last kept against its first dropped candidate; the boundary of A where its last pick was taken; a row's best against its second best
#: where only M brought the taken word in) and >= 2e-4 between neighbouring final scores.  Measured on the CPU, boundary / final:
#:   k4_c1  seed 2 1.38e-3 / 3.49e-3, seed 5 4.21e-3 / 1.44e-2        k4_c2  seed 101 1.25e-3 / 1.85e-2, seed 33 1.22e-3 / 2.95e-2
#:   k6_c3  seed 41 1.07e-3 / 1.21e-2, seed 3 3.44e-3 / 4.28e-2       k4_c2_n2_banned  seed 3 1.04e-3 / 2.32e-2, seed 5 4.43e-3 / 2.75e-3
#: "k4_c2" also compares the device's plain beam with the words (test 4), so there history_ref's plain beam keeps the same margins
#: (seed 101 1.96e-3 / 3.89e-4, seed 33 2.72e-3 / 5.57e-4); elsewhere the plain beam only supplies the words, on the CPU.
REF_CASES = {"k4_c1": dict(K=4, C=1), "k4_c2": dict(K=4, C=2, plain=True), "k6_c3": dict(K=6, C=3), "k4_c2_n2_banned": dict(K=4, C=2, ruled=True)}
REF_SEEDS = {"k4_c1": {1: 2, 2: 5}, "k4_c2": {1: 101, 2: 33}, "k6_c3": {1: 41, 2: 3}, "k4_c2_n2_banned": {1: 3, 2: 5}}
_cache = {}


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _select(lib, L, scores, klive, hist, hist_len, first, words, n_words, Cmax, end_id):
    B, K, Vk = scores.shape
    values = torch.full((B, K), float("nan"), device="cuda"); indices = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    work = torch.full((B, K, Vk), 123.0, device="cuda")
    req = L.BeamRequired(max_required=Cmax, words=words.data_ptr() if Cmax else None, n_words=n_words.data_ptr() if Cmax else None)
    L.check(lib.sat_beam_required_select(L.ptr(scores), L.ptr(klive), B, K, Vk, L.ptr(hist), hist.shape[1], int(hist_len), int(first), C.byref(req),
                                         int(end_id), L.ptr(work), L.ptr(values), L.ptr(indices), L.stream_ptr()), "sat_beam_required_select")
    return values, indices


@pytest.mark.parametrize("Vk", [83, 257, 1030])
def test_required_select_kernel_bit_for_bit(Vk):
    """1. B = 5, K = 6, C in {0, 1, 3, 8} with ragged n_words (0 included, out-of-range counts clamped), both first_step values, the last step,
    and history lengths 0, 8 and one past the table (clamped): indices equal and values equal bit for bit to required_ref.select; two runs
    give the same bits.  klive is 6, 4, 0 (or -2), 9 (clamped) and 3.  Image 0: row 0 has said every word and its best word is END
    (taken), row 1 has said nothing, its first word is at -inf (dropped from R) and its second word is the best score of the image (in A,
    R and M at once), row 2 has said the first word only and its best word is END (held back while C > 1).  Image 1 has no words next
    to constrained ones: its picks are sat_topk's.  Image 3: two words tie exactly in every row (ties inside a row and across rows of one
    bank) and a required word is at -inf in two rows.  Image 4 has two finite candidates for three picks, an id outside [0, V) and a
    negative id among its words."""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    B, K, END, stride = 5, 6, 2, 10
    g = torch.Generator().manual_seed(500 + Vk)
    base = torch.randn(B, K, Vk, generator=g) * 3.0 - 8.0
    base[torch.rand(B, K, Vk, generator=g) < 0.1] = float("-inf")
    words = torch.tensor([[10 + 3 * c + b for c in range(8)] for b in range(B)], dtype=torch.int32)
    words[4, 2] = Vk + 5; words[4, 3] = -1
    hist = torch.randint(40, 80, (B * K, stride), generator=g).to(torch.int32)      # no required word (those are < 40)
    hist[0, :8] = words[0]                                  # image 0, row 0: everything said
    hist[2, 3] = words[0, 0]                                # image 0, row 2: the first word only
    hist[3 * K + 1, 5] = words[3, 1]; hist[3 * K + 4, 0] = words[3, 0]; hist[3 * K + 4, 7] = words[3, 2]
    base[0, 0, END] = 70.0; base[0, 2, END] = 65.0
    base[0, 1, words[0, 0]] = float("-inf"); base[0, 1, words[0, 1]] = 60.0
    base[3, :, 7] = 50.0; base[3, :, Vk - 1] = 50.0
    base[3, 2:4, words[3, 1]] = float("-inf")
    base[4] = float("-inf"); base[4, 0, 5] = -1.0; base[4, 1, 9] = -2.0
    checked = 0
    for Cmax in (0, 1, 3, 8):
        n_words = torch.tensor([Cmax, 0, max(Cmax - 1, 0), Cmax + 5, Cmax], dtype=torch.int32)
        if Cmax == 8:
            n_words[2] = -3                                 # clamped to 0
        wd = words[:, :max(Cmax, 1)].contiguous()
        for first, hist_len in ((0, 8), (1, 0), (1, 8), (0, stride + 7), (2, 8), (3, 0)):      # first & 1: row 0 alone; first & 2: the last step
            klive = torch.tensor([6, 4, -2 if first & 1 else 0, 9, 3], dtype=torch.int32)
            args = (base.cuda().contiguous(), klive.cuda(), hist.cuda().contiguous(), hist_len, first, wd.cuda(), n_words.cuda(), Cmax, END)
            values, indices = _select(lib, L, *args)
            v2, i2 = _select(lib, L, *args)
            assert torch.equal(values.view(torch.int32), v2.view(torch.int32)) and torch.equal(indices, i2)
            wv, wi = RR.select(base.numpy(), klive.numpy(), hist.numpy(), hist_len, wd.numpy()[:, :Cmax], n_words.numpy(), first, END)
            gv, gi = values.cpu().numpy(), indices.cpu().numpy()
            assert np.array_equal(gi, wi), (Cmax, first, hist_len, gi, wi)
            assert np.array_equal(gv.view(np.int32), wv.view(np.int32)), (Cmax, first, hist_len)
            checked += 1
            assert (wi[2] == -7).all() and np.isnan(wv[2]).all()                    # no live row: untouched
            # image 1 has no words: sat_topk's picks on its live rows
            n1 = Vk if first & 1 else 4 * Vk
            tv = torch.empty(4, device="cuda"); ti = torch.empty(4, dtype=torch.int32, device="cuda")
            x1 = base[1].reshape(-1)[:n1].cuda().contiguous()
            L.check(lib.sat_topk(L.ptr(x1), L.ptr(torch.empty_like(x1)), n1, 4, L.ptr(tv), L.ptr(ti), L.stream_ptr()), "sat_topk")
            assert torch.equal(ti.cpu(), indices[1, :4].cpu()) and torch.equal(tv.cpu().view(torch.int32), values[1, :4].cpu().view(torch.int32))
            # image 4: two finite candidates, then nothing is left
            assert np.isneginf(wv[4, 2]) and wi[4].tolist()[:3] == ([5, 0, 0 if Cmax else 1] if first & 1 else [5, Vk + 9, 0])
            if Cmax and first == 0 and hist_len >= 8:        # the planted cases did what they are there for
                picks0 = wi[0].tolist()
                assert picks0[0] == END                     # the complete row's END: the fullest bank goes first
                assert 1 * Vk + int(words[0, 0]) not in picks0                       # at -inf: not a candidate
                assert (2 * Vk + END in picks0) == (Cmax == 1)                       # held back while a word is missing
                if Cmax > 1:
                    assert picks0.count(1 * Vk + int(words[0, 1])) == 1              # in A, R and M: one candidate
    assert checked == 24


# ------------------------------------------------------------------------------------------------ 2. off is today's search
def _raw_required(dec, hp, ann, K, hist, req, with_met=True, S_=S):
    """sat_beam_search_required on zeroed buffers, as TC._raw calls its neighbours; "req_met" starts at -9"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    B, Lc, D = ann.shape
    dims = Dk.decoder_dims(B, K, 2, Lc, D, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=int(hp.decoder_layers))
    w, keep = dec._params_struct()
    i32 = dict(dtype=torch.int32, device="cuda"); f32 = dict(dtype=torch.float32, device="cuda")
    o = dict(tok_in=torch.zeros(S_ + 2, B, K, **i32), prev_row=torch.zeros(S_ + 2, B, K, **i32), alpha_hist=torch.zeros(S_ + 1, B, K, Lc, **f32),
             fin_count=torch.zeros(B, **i32), fin_step=torch.zeros(B, K, **i32), fin_row=torch.zeros(B, K, **i32),
             fin_score=torch.zeros(B, K, **f32), fin_mean=torch.zeros(B, K, **f32))
    met = torch.full((B,), -9, **i32)
    tarr = (C.c_float * len(TEMPS))(*TEMPS)
    ids = (C.c_int32 * 4)(*[int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    outs = [L.ptr(o[k]) for k in ("tok_in", "prev_row", "alpha_hist", "fin_count", "fin_step", "fin_row", "fin_score", "fin_mean")]
    nbytes = lib.sat_beam_search_required_workspace_bytes(C.byref(dims), K, S_, req.max_required if req is not None else 0)
    assert nbytes == lib.sat_beam_search_history_workspace_bytes(C.byref(dims), K, 0, S_) > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    L.check(lib.sat_beam_search_required(C.byref(dims), C.byref(w), L.ptr(ann), K, S_, tarr, len(TEMPS), ids, None, None,
                                         C.byref(hist) if hist is not None else None, C.byref(req) if req is not None else None, *outs,
                                         L.ptr(met) if with_met else None, L.ptr(ws), nbytes, L.stream_ptr()), "sat_beam_search_required")
    torch.cuda.synchronize()
    return o, met


@pytest.mark.parametrize("layers", [1, 2])
def test_required_off_is_todays_search_bit_for_bit(layers):
    """2. required = NULL, max_required = 0 (req_met NULL and never written) and every n_words[b] = 0 (through the new kernels) against
    sat_beam_search_history without a rule and with no_repeat_ngram = 2: every back-trace buffer equal, at beams 1 and 4"""
    from sat_amd import _lib as L
    dec, hp, ann = TC._setup(layers)
    words = torch.full((9, 2), 11, dtype=torch.int32, device="cuda"); zeros = torch.zeros(9, dtype=torch.int32, device="cuda")
    for K in (1, 4):
        for hist in (None, L.BeamHistory(no_repeat_ngram=2)):
            want = TH._raw_history(dec, hp, ann, K, None, None, hist)
            assert int(want["fin_count"].min()) >= 1
            for name, req, with_met in (("null", None, False), ("zero", L.BeamRequired(max_required=0), False),
                                        ("no words", L.BeamRequired(max_required=2, words=words.data_ptr(), n_words=zeros.data_ptr()), True)):
                got, met = _raw_required(dec, hp, ann, K, hist, req, with_met)
                for k in want:
                    assert torch.equal(got[k], want[k]), (K, hist is not None, name, k)
                assert met.tolist() == ([0] * 9 if name == "no words" else [-9] * 9)


# ------------------------------------------------------------------------------------------------ the searches under test
def _batched(layers, seed, K, **kw):
    """beam_decode_batched(LN, return_all) on the seeded decoder, computed once per setting and left unchanged"""
    key = (layers, seed, K, tuple(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _cache:
        dec, _, ann = TC._setup(layers, seed=seed)
        _cache[key] = dec.beam_decode_batched(ann, HW, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True, **kw)
    return _cache[key]


def _cpu_inputs(layers, seed):
    dec, hp, ann = TC._setup(layers, seed=seed)
    sd = {k: v.detach().cpu().clone() for k, v in dec.state_dict().items()}
    return sd, hp, ann.cpu().reshape(9, 3, 4, 32).permute(0, 3, 1, 2).contiguous()


def _margins(m):
    boundary = [g for g in m["boundary"] if g is not None]
    final = [g for gaps in m["final"] for g in gaps]
    return min(boundary), len(boundary), min(final) if final else float("inf"), len(final)


def _reference(layers, case):
    """(seed, required words, rules, the plain and the required result of the CPU references, required_ref's info), once per case; the
    words of an image are the lowest ids that no hypothesis of history_ref's plain beam at the same K says: its coverage is 0"""
    key = ("ref", layers, case)
    if key not in _cache:
        c = REF_CASES[case]
        K, seed = c["K"], REF_SEEDS[case][layers]
        sd, hp, ann_img = _cpu_inputs(layers, seed)
        kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True)
        mp, m, info, rules = {}, {}, {}, {}
        with torch.no_grad():
            plain = HR.beam_search(sd, hp, ann_img, margins=mp, **kw)
            req = TR.unsaid_words(plain, hp, c["C"])
            if c.get("ruled"):
                rules = dict(no_repeat_ngram=2, banned=TR.ruled_banned(RR.beam_search(sd, hp, ann_img, required=req, **kw), hp, req))
            want = RR.beam_search(sd, hp, ann_img, required=req, margins=m, info=info, **kw, **rules)
        pb, _, pf, _ = _margins(mp)
        b, nb, f, nf = _margins(m)
        print("%s layers=%d seed=%d margins: plain boundary %.3e final %.3e; required boundary %.3e over %d selections, final %.3e over %d neighbours"
              % (case, layers, seed, pb, pf, b, nb, f, nf))
        assert b >= 1e-3 and f >= 2e-4 and (not c.get("plain") or (pb >= 1e-3 and pf >= 2e-4))
        _cache[key] = (seed, req, rules, plain, want, info)
    return _cache[key]


@pytest.mark.parametrize("layers", [1, 2])
def test_mixed_batch_leaves_the_images_without_words_alone(layers):
    """2. words for the even images only: the odd images return the unconstrained search's lists, captions exact and values within 1e-5
    (the project's batched bound); the even ones differ from it"""
    seed, req, _, _, _, _ = _reference(layers, "k4_c2")
    mixed = [r if b % 2 == 0 else [] for b, r in enumerate(req)]
    plain = _batched(layers, seed, 4)
    got = _batched(layers, seed, 4, required=mixed)
    odd = lambda res: tuple([part[b] for b in range(1, 9, 2)] for part in res)
    TC._close(odd(plain), odd(got), 1e-5)
    assert all(got[0][b] != plain[0][b] for b in range(0, 9, 2))


# ------------------------------------------------------------------------------------------------ 3. against required_ref
@pytest.mark.parametrize("case", list(REF_CASES))
@pytest.mark.parametrize("layers", [1, 2])
def test_against_the_cpu_reference_search(layers, case):
    """3. captions and list order identical, values within 1e-4 (the GPU-vs-CPU bound); the margins of both references are asserted in
    _reference.  The ruled case adds no_repeat_ngram = 2 and three banned ids (<UNK> and the two commonest words of the un-ruled result
    that no image requires)."""
    seed, req, rules, plain, want, info = _reference(layers, case)
    K, Cn = REF_CASES[case]["K"], REF_CASES[case]["C"]
    assert all(len(r) == Cn for r in req) and info["req_met"] == [Cn] * 9
    assert all(RR.count_required(c, req[b]) == 0 for b in range(9) for c in plain[0][b])        # the plain beam's coverage is 0
    got = _batched(layers, seed, K, required=req, **rules)
    want = (want[0], want[1], [[a.reshape(-1, *HW) for a in al] for al in want[2]], want[3])
    TC._close(want, got, 1e-4)
    assert all(RR.count_required(c, req[b]) == Cn for b in range(9) for c in got[0][b])
    if rules:
        assert len(rules["banned"]) == 3 and int(_cpu_inputs(layers, seed)[1].vocab_stoi["<UNK>"]) in rules["banned"]
        assert not any(t in rules["banned"] for caps in got[0] for cap in caps for t in cap)
        assert not any(HR.repeats_ngram(cap, 2) for caps in got[0] for cap in caps)
        assert got[0] != _batched(layers, seed, K, required=req)[0]                              # the rules change this search


# ------------------------------------------------------------------------------------------------ 4. properties of the device result
@pytest.mark.parametrize("layers", [1, 2])
def test_properties_of_the_device_result(layers):
    """4. K = 4, two words per image that the plain beam never says.  The returned caption of 9 of 9 images contains its words
    (required_coverage == 1.0, the plain search's is 0.0), req_met == C_b, fin_count >= 1, every hypothesis left in the lists reaches
    req_met (recounted on the host from sat_beam_hypotheses), and fin_score is the teacher-forced sum of the words' log-probabilities
    within 1e-4: the allocation does not leak into the scores.  The sum is required_ref.sequence_logprob, which is
    group_ref.sequence_logprob started from the beam's own initial state (the reshape of the initial state depends on the row count, so at
    beamk = 4 the one-row sum is another model's; at beamk = 1 the two are the same function).  A hypothesis that ended before the last
    step closed with <END>; for one that ended at the last step the buffers do not say whether <END> or the cut closed it, so its closing
    word is the one required_ref recorded for the same entry of the list (the lists agree entry by entry: test 3 and the margins).
    max_gen_length = C_b still meets every word, by the cut; max_gen_length = C_b - 1 is refused."""
    import sat_amd  # noqa: F401
    from sat_amd import constraints as Cn, evaluation as E
    K = 4
    seed, req, _, _, _, info = _reference(layers, "k4_c2")
    dec, hp, ann = TC._setup(layers, seed=seed)
    sd, _, ann_img = _cpu_inputs(layers, seed)
    END = int(hp.vocab_stoi["<END>"])
    best = dec.beam_decode_batched(ann, HW, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", required=req)
    plain = dec.beam_decode_batched(ann, HW, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN")
    assert Cn.required_coverage(best[0], req) == [1.0] * 9 and Cn.required_coverage(plain[0], req) == [0.0] * 9
    o = dec._beam_search_device(ann, K, S, TEMPS, "beam", 3, None, None, None, None, False, required=req)
    hyp, hyp_len = E.finished_hypotheses(o, dec.pad_idx)
    hyp, hyp_len = hyp.cpu().tolist(), hyp_len.cpu().tolist()
    o = {k: v.cpu() for k, v in o.items() if k != "ws"}
    assert o["req_met"].tolist() == [2] * 9 and int(o["fin_count"].min()) >= 1 and int(o["fin_count"].max()) <= K
    worst, scored = 0.0, 0
    for b in range(9):
        kept = [e for e, (_, n) in zip(info["said"][b], info["ended"][b]) if n == info["req_met"][b]]    # required_ref's list after its compaction
        assert len(kept) == int(o["fin_count"][b])
        for f in range(int(o["fin_count"][b])):
            said = hyp[b][f][:hyp_len[b][f]]
            assert RR.count_required(said, req[b]) == int(o["req_met"][b]), (b, f, said)
            step, cur = int(o["fin_step"][b, f]), int(o["fin_row"][b, f])
            assert step == len(said) and kept[f][0][:-1] == said
            closing = END if step < S else kept[f][0][-1]
            for s in range(step, 1, -1):
                cur = int(o["prev_row"][s, b, cur])
            lp = RR.sequence_logprob(sd, hp, ann_img[b], said + [closing], TEMPS, K, cur)  # cur: the slot the first word was kept in
            err = abs(lp - float(o["fin_score"][b, f])) / max(1.0, abs(lp))
            worst, scored = max(worst, err), scored + 1
            assert err <= 1e-4, (b, f, lp, float(o["fin_score"][b, f]))
    print("fin_score against the teacher-forced sum of log-probabilities: %d hypotheses, worst relative error %.2e" % (scored, worst))
    assert scored == int(o["fin_count"].sum())
    short = dec._beam_search_device(ann, K, 2, TEMPS, "beam", 3, None, None, None, None, False, required=req)
    assert short["req_met"].cpu().tolist() == [2] * 9 and int(short["fin_count"].min()) >= 1
    with pytest.raises(ValueError, match="max_gen_length"):
        dec._beam_search_device(ann, K, 1, TEMPS, "beam", 3, None, None, None, None, False, required=req)


# ------------------------------------------------------------------------------------------------ 5. the public surface
@pytest.mark.parametrize("layers", [1, 2])
def test_mbr_and_ln_pick_among_the_compacted_lists(layers):
    """5. rescore_method "LN" and "MBR" (the small corpus of tests/test_gpu_mbr.py) over the lists the required words left: every
    returned hypothesis of every image contains its words, and MBR returns the hypotheses of the un-rescored search"""
    import test_gpu_mbr as TM
    seed, req, _, _, _, _ = _reference(layers, "k4_c2")
    dec, hp, ann = TC._setup(layers, seed=seed)
    rc, _, _ = TM._e2e_corpus()
    kw = dict(beamk=4, max_gen_length=S, temperature=TEMPS, required=req, return_all=True)
    base = dec.beam_decode_batched(ann, HW, rescore_method=None, **kw)
    for method, extra in (("LN", {}), ("MBR", dict(mbr_corpus=rc, mbr_reward=(0.5, 0.5), mbr_alpha=1.0))):
        every = dec.beam_decode_batched(ann, HW, rescore_method=method, **extra, **kw)
        for b in range(9):
            assert sorted(map(tuple, every[0][b])) == sorted(map(tuple, base[0][b])) and len(every[0][b]) >= 1
            assert all(RR.count_required(c, req[b]) == len(req[b]) for c in every[0][b])
            assert all(every[1][b][i] >= every[1][b][i + 1] for i in range(len(every[1][b]) - 1))


@pytest.mark.parametrize("precision,layers", [("fp32", 1), ("bf16", 2)])
def test_public_surface_takes_the_required_words(precision, layers):
    """5. SAT.caption(required=...) with ids and with a string, shared and per image (one image without words), deep output, one layer in
    fp32 and two layers in bf16: every caption contains its words; caption_tokens, val_batch_stats and caption_image take the keyword
    and their selected captions have coverage 1.0"""
    import sat_amd  # noqa: F401
    from sat_amd import constraints as Cn, model as M
    from oracle import prng, sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16,
                decoder_dim=40, deep_output=True, decoder_layers=layers, val_beamk=3, val_max_len=7)
    torch.manual_seed(5)
    hp = O.default_hparams(**over)
    names = {"dog": 11, "frisbee": 23, "grass": 31}
    for word, t in names.items():                           # three ordinary ids get names a user would type
        hp.vocab_stoi[word], hp.vocab_itos[t] = t, word
    model = M.SAT(**vars(hp)).cuda()
    model.set_precision(precision)
    img = torch.from_numpy(prng.uniform((4, 3, 64, 64), 41, 0.0, 1.0)).cuda()
    caps, lengths = prng.captions(4, 3, 9, 60, 42, min_len=3)
    caps, lengths = torch.from_numpy(caps).cuda(), torch.from_numpy(lengths)
    kw = dict(beamk=4, max_gen_length=7, temperature=1.0, rescore_method="LN")
    plain = model.caption(img, **kw)
    for required in ([11, 23], "dog frisbee", [[11], "frisbee grass", [], [31, 23, 11]], ["dog", "dog", "grass dog", ""]):
        captions, scores, _, ppl = model.caption(img, required=required, **kw)
        assert Cn.required_coverage(captions, required, model.hp.vocab_stoi) == [1.0] * 4, required
    assert model.caption(img, required=[], **kw)[0] == plain[0] and model.caption(img, required=None, **kw)[1] == plain[1]
    per_image = [[11], "frisbee grass", [], [31, 23, 11]]
    captions = model.caption(img, required=per_image, **kw)[0]
    assert captions[2] == plain[0][2]                       # the image without words
    tok, ln, _, _ = model.caption_tokens(img, required=per_image, **kw)
    tok, ln = tok.cpu().tolist(), ln.cpu().tolist()
    assert Cn.required_coverage([tok[b][:ln[b]] for b in range(4)], per_image, model.hp.vocab_stoi) == [1.0] * 4
    stats = model.val_batch_stats((img, caps, lengths), required=per_image, **kw).metrics()
    assert set(stats) == set(model.val_batch((img, caps, lengths), required=per_image, **kw))
    words = model.caption_image([np.zeros((80, 80, 3), np.uint8)], beamk=4, max_gen_length=7, rescore_method="LN", required="grass dog")
    assert Cn.required_coverage(words[1], "grass dog") == [1.0] and Cn.required_coverage(words[0], "grass dog", model.hp.vocab_stoi) == [1.0]
