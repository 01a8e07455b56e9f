"""GPU: the diverse (group) beam search of the batched caption search ("Diverse beam search").  Shapes, helpers and models of
tests/test_gpu_constrained_search.py: V = 83 (every kernel's tail), 9 images, L = 12, max_gen_length = 9, temperatures [1.0, 0.7], one and
two LSTM layers; beams K = 4 (G = 2, 4) and K = 6 (G = 2, 3).

The selection kernel is checked bit for bit (its penalty is two fp32 roundings that numpy float32 restates), the search against the CPU
reference tests/group_ref.py within the project's GPU-vs-CPU bound 1e-4 and against the plain search at beamk = K / G within its
batched-vs-loop bound 1e-5.  Every model seed below was chosen on the CPU with group_ref / history_ref alone so that no pick and no final
order of the reference rests on a near-tie; the tests assert those margins again."""
import ctypes as C

import numpy as np
import pytest
import torch

import group_ref as GR
import history_ref as HR
import test_gpu_constrained_search as TC
import test_gpu_search_history as TH

pytestmark = pytest.mark.gpu

V, S, HW, TEMPS = TC.V, TC.S, TC.HW, TC.TEMPS
#: test 3: history_ref.beam_search at beamk 1 and 2 keeps >= 1e-3 at every selection and >= 2e-4 between final scores (measured: seed 5
#: boundary 1.6e-3 / 2.7e-3, final 7.1e-3; seed 3 boundary 8.2e-2 / 2.3e-3, final 3.3)
SMALL_SEEDS = {1: 5, 2: 3}
#: test 4, lambda = 0.5 at (K, G) = (4, 2) and (6, 3): group_ref's margins on the penalised values (measured: seed 31 boundary 1.9e-3 /
#: 1.3e-3, final 3.1e-3 / 1.4e-3; seed 20 boundary 1.2e-3 / 1.2e-3, final 1.6e-3 / 1.6e-3)
REF_SEEDS = {1: 31, 2: 20}
#: test 4, no_repeat_ngram = 2 with <UNK> (80) and the two commonest words of the un-ruled grouped result banned, (K, G) = (4, 2),
#: lambda = 0.5 (measured: seed 17 boundary 1.3e-3, final 1.3e-3; seed 16 boundary 1.5e-3, final 2.9e-3)
RULED = {1: dict(seed=17, banned=[22, 65, 80]), 2: dict(seed=16, banned=[25, 52, 80])}
#: test 5, lambda = 1e4 with one row per group at K = 4: the plain beam and the grouped one both keep the margins above (measured: seed 7
#: plain boundary 1.4e-3 final 2.0e-3, grouped 1.2e-3 / 1.5e-3; seed 33 plain 2.7e-3 / 5.6e-4, grouped 1.4e-3 / 1.8e-3), and group_ref's
#: distinct-1 and distinct-2 are strictly above history_ref's plain beam on 9 of 9 images for both seeds
BITE_SEEDS = {1: 7, 2: 33}
BITE_STRICT = 9
_cache = {}


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _restate(scores, klive, G, first, lam):
    """numpy float32: (values, indices) of sat_beam_group_select; slots no group writes keep NaN / -7"""
    B, K, Vk = scores.shape
    Kg = K // G
    values = np.full((B, K), np.nan, np.float32); indices = np.full((B, K), -7, np.int32)
    lam = np.float32(lam)
    for b in range(B):
        kept = []
        for g in range(G):
            k = int(np.clip(klive[b, g], 0, Kg))
            if k == 0:
                continue
            x = scores[b, g * Kg:(g + 1) * Kg].reshape(-1)[:Vk if first else k * Vk]
            c = np.bincount(np.asarray(kept, np.int64), minlength=Vk).astype(np.float32)
            pen = x - np.tile(lam * c, len(x) // Vk)                  # float32 product, then float32 difference
            assert pen.dtype == np.float32
            pick = np.argsort(-pen, kind="stable")[:k]                 # descending, ties to the lower flat index, -inf last in index order
            values[b, g * Kg:g * Kg + k] = x[pick]; indices[b, g * Kg:g * Kg + k] = pick
            kept += (pick % Vk).tolist()
    return values, indices


def _select(lib, L, scores, klive, G, first, lam):
    B, K, Vk = scores.shape
    values = torch.full((B, K), float("nan"), device="cuda"); indices = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    work = torch.full((B, K, Vk), 123.0, device="cuda")
    L.check(lib.sat_beam_group_select(L.ptr(scores), L.ptr(klive), B, K, G, Vk, int(first), float(lam), L.ptr(work), L.ptr(values), L.ptr(indices),
                                      L.stream_ptr()), "sat_beam_group_select")
    return values, indices


@pytest.mark.parametrize("Vk", [83, 257, 1030])
def test_group_select_kernel_bit_for_bit(Vk):
    """1. B = 5, K = 6, G in {1, 2, 3, 6}, both first_step values, lambda in {0, 0.5, 1e4}: indices equal and values equal bit for bit
    to the numpy float32 restatement.  klive is ragged per group (0, full, partial, and out-of-range values that are clamped); image 3
    has a group with fewer finite candidates than picks and groups of nothing but -inf; every image has -inf entries; two words tie
    exactly in every row of image 0 (the tie rule inside and across rows; c[v] > 1 for the later groups), in image 1 the best word
    less lambda = 0.5 equals the second best (a tie between a penalised and an unpenalised candidate), image 2 has two equal rows;
    two runs give the same bits."""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    B, K = 5, 6
    g = torch.Generator().manual_seed(300 + Vk)
    base = torch.randn(B, K, Vk, generator=g) * 3.0 - 8.0
    base[torch.rand(B, K, Vk, generator=g) < 0.1] = float("-inf")
    base[0, :, 7] = 50.0                                   # the best word of every row of image 0, the same float in all of them
    base[0, :, Vk - 1] = 50.0                              # and a second one: ties inside a row as well
    base[1, :, 11] = 40.0; base[1, :, 12] = 39.5           # at lambda = 0.5 word 11, kept once, ties with word 12 exactly (G = 6)
    base[2, 0, :] = base[2, 1, :]                          # two equal rows: every candidate ties across rows
    base[3, 2:, :] = float("-inf"); base[3, 2, 5] = -1.0   # rows 2..5 of image 3: one finite candidate, the rest -inf
    checked = picks = 0
    for G in (1, 2, 3, 6):
        Kg = K // G
        klive = torch.tensor([[(b + 2 * gi) % (Kg + 1) for gi in range(G)] for b in range(B)], dtype=torch.int32)
        klive[0, :] = Kg; klive[1, :] = Kg; klive[3, :] = Kg
        klive[4, 0] = Kg + 3                               # clamped to Kg
        if G > 1:
            klive[4, 1] = -2                               # clamped to 0
        assert (klive == 0).any() or G == 1
        for first in (0, 1):
            for lam in (0.0, 0.5, 1e4):
                sc = base.cuda().contiguous(); kl = klive.cuda().contiguous()
                values, indices = _select(lib, L, sc, kl, G, first, lam)
                v2, i2 = _select(lib, L, sc, kl, G, first, lam)
                assert torch.equal(values.view(torch.int32), v2.view(torch.int32)) and torch.equal(indices, i2)
                wv, wi = _restate(base.numpy(), klive.numpy(), G, first, lam)
                gv, gi = values.cpu().numpy(), indices.cpu().numpy()
                assert np.array_equal(gi, wi), (G, first, lam, gi, wi)
                assert np.array_equal(gv.view(np.int32), wv.view(np.int32)), (G, first, lam)
                checked += 1; picks += int((wi >= 0).sum())
                if G > 1 and not first and lam > 0:        # the planted ties did what they are there for
                    assert wi[0, :Kg].tolist()[:2] == [7, Vk - 1][:Kg] and np.isneginf(wv[3]).any()
                    if G == 6 and lam == 0.5:              # 40 - 0.5 == 39.5: the tie goes to the lower index, the penalised word
                        assert wi[1].tolist()[:2] == [11, 11] and wv[1, 1] == 40.0
    assert checked == 24 and picks > 300


# ------------------------------------------------------------------------------------------------ 2. off is today's search
def _raw_groups(dec, hp, ann, K, smp, con, hist, grp):
    """sat_beam_search_groups on zeroed buffers, as TC._raw calls its neighbours"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    B, Lc, D = ann.shape
    dims = Dk.decoder_dims(B, K, 2, Lc, D, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=int(hp.decoder_layers))
    w, keep = dec._params_struct()
    i32 = dict(dtype=torch.int32, device="cuda"); f32 = dict(dtype=torch.float32, device="cuda")
    o = dict(tok_in=torch.zeros(S + 2, B, K, **i32), prev_row=torch.zeros(S + 2, B, K, **i32), alpha_hist=torch.zeros(S + 1, B, K, Lc, **f32),
             fin_count=torch.zeros(B, **i32), fin_step=torch.zeros(B, K, **i32), fin_row=torch.zeros(B, K, **i32),
             fin_score=torch.zeros(B, K, **f32), fin_mean=torch.zeros(B, K, **f32))
    tarr = (C.c_float * len(TEMPS))(*TEMPS)
    ids = (C.c_int32 * 4)(*[int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    outs = [L.ptr(o[k]) for k in ("tok_in", "prev_row", "alpha_hist", "fin_count", "fin_step", "fin_row", "fin_score", "fin_mean")]
    nbytes = lib.sat_beam_search_groups_workspace_bytes(C.byref(dims), K, grp.groups if grp is not None else 0, S)
    assert nbytes >= lib.sat_beam_search_history_workspace_bytes(C.byref(dims), K, 0, S) > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    L.check(lib.sat_beam_search_groups(C.byref(dims), C.byref(w), L.ptr(ann), K, S, tarr, len(TEMPS), ids, C.byref(smp) if smp is not None else None,
                                       C.byref(con) if con is not None else None, C.byref(hist) if hist is not None else None,
                                       C.byref(grp) if grp is not None else None, *outs, L.ptr(ws), nbytes, L.stream_ptr()), "sat_beam_search_groups")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("layers", [1, 2])
def test_groups_off_is_todays_search_bit_for_bit(layers):
    """2. groups = NULL, {0, 0}, {1, 0.5} and {1, 1e4} against sat_beam_search_constrained (no rule) and sat_beam_search_history
    (no_repeat_ngram = 2): every back-trace buffer equal, at beams 1 and 4"""
    from sat_amd import _lib as L
    dec, hp, ann = TC._setup(layers)
    for K in (1, 4):
        for hist in (None, L.BeamHistory(no_repeat_ngram=2)):
            want = TC._raw(dec, hp, ann, K, "constrained") if hist is None else TH._raw_history(dec, hp, ann, K, None, None, hist)
            assert int(want["fin_count"].min()) >= 1
            for grp in (None, L.BeamGroups(), L.BeamGroups(groups=1, diversity_penalty=0.5), L.BeamGroups(groups=1, diversity_penalty=1e4)):
                got = _raw_groups(dec, hp, ann, K, None, None, hist, grp)
                for k in want:
                    assert torch.equal(got[k], want[k]), (K, hist is not None, grp is not None and (grp.groups, grp.diversity_penalty), k)


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
    return min(boundary), len(boundary), min(final) if final else float("inf"), len(final)     # beamk = 1: one hypothesis, no neighbour


# ------------------------------------------------------------------------------------------------ 3. lambda = 0
@pytest.mark.parametrize("K,G", [(4, 2), (4, 4), (6, 3)])
@pytest.mark.parametrize("layers", [1, 2])
def test_no_penalty_is_independent_small_beams(layers, K, G):
    """3. lambda = 0: each image's return_all list is G copies of the plain search at beamk = K / G.  Captions identical; values within
    1e-5, the batched-vs-loop bound (the GEMMs see another row count, so bit equality is not claimed).  The plain search's own margins
    (history_ref on the CPU) are asserted: boundary >= 1e-3, final >= 2e-4."""
    seed = SMALL_SEEDS[layers]
    sd, hp, ann_img = _cpu_inputs(layers, seed)
    m = {}
    with torch.no_grad():
        HR.beam_search(sd, hp, ann_img, beamk=K // G, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True, margins=m)
    b, nb, f, nf = _margins(m)
    print("plain beamk=%d margins: boundary %.3e over %d selections, final %.3e over %d neighbours" % (K // G, b, nb, f, nf))
    assert b >= 1e-3 and f >= 2e-4
    small = _batched(layers, seed, K // G)
    got = _batched(layers, seed, K, beam_groups=G, diversity_penalty=0.0)
    want = tuple([[x for x in img for _ in range(G)] for img in part] for part in small)
    assert all(len(c) == K for c in got[0])
    TC._close(want, got, 1e-5)


# ------------------------------------------------------------------------------------------------ 4. against group_ref
REF_CASES = {"k4_g2": dict(K=4, G=2), "k6_g3": dict(K=6, G=3), "k4_g2_n2_banned": dict(K=4, G=2, ruled=True)}


@pytest.mark.parametrize("case", list(REF_CASES))
@pytest.mark.parametrize("layers", [1, 2])
def test_against_the_cpu_reference_search(layers, case):
    """4. lambda = 0.5: captions and list order identical, values within 1e-4 (the GPU-vs-CPU bound); group_ref's own margins, taken on
    the penalised values of every group's selection, prove that no pick and no final order rests on a near-tie (boundary >= 1e-3,
    final >= 2e-4).  Measured on the CPU: the figures next to REF_SEEDS and RULED above."""
    c = REF_CASES[case]
    K, G = c["K"], c["G"]
    seed, rules = REF_SEEDS[layers], {}
    if c.get("ruled"):
        seed, rules = RULED[layers]["seed"], dict(no_repeat_ngram=2, banned=RULED[layers]["banned"])
    sd, hp, ann_img = _cpu_inputs(layers, seed)
    if rules:
        assert int(hp.vocab_stoi["<UNK>"]) in rules["banned"] and len(rules["banned"]) == 3
    m = {}
    with torch.no_grad():
        want = GR.beam_search(sd, hp, ann_img, beamk=K, beam_groups=G, diversity_penalty=0.5, max_gen_length=S, temperature=TEMPS, rescore_method="LN",
                              return_all=True, margins=m, **rules)
    b, nb, f, nf = _margins(m)
    print("reference margins: boundary %.3e over %d selections, final %.3e over %d neighbours" % (b, nb, f, nf))
    assert b >= 1e-3 and f >= 2e-4
    got = _batched(layers, seed, K, beam_groups=G, diversity_penalty=0.5, **rules)
    want = (want[0], want[1], [[a.reshape(-1, *HW) for a in al] for al in want[2]], want[3])
    TC._close(want, got, 1e-4)
    assert got[0] != _batched(layers, seed, K, **rules)[0]               # the penalty changes this search
    if rules:
        assert not any(t in rules["banned"] for caps in got[0] for cap in caps for t in cap)
        assert not any(HR.repeats_ngram(cap, 2) for caps in got[0] for cap in caps)


# ------------------------------------------------------------------------------------------------ 5. properties with bite
def _kept_words(o, b, K, END):
    """one row per group: step -> the word every live group kept at that step, from the back-trace buffers"""
    fin = {int(o["fin_row"][b, f]): int(o["fin_step"][b, f]) for f in range(int(o["fin_count"][b]))}
    assert sorted(fin) == list(range(K))                                # every group finished exactly once, fin_row is its image-level row
    steps = {}
    for g, last in fin.items():
        for s in range(last + 1):
            w = int(o["tok_in"][s + 1, b, g])
            if s == last:
                w = w if (s == S and w != 0) else END                   # cut at max_gen_length: the dropped word; else the closing <END>
            steps.setdefault(s, []).append((g, w))
    return steps, fin


@pytest.mark.parametrize("layers", [1, 2])
def test_properties_with_bite(layers):
    """5. lambda = 1e4, K = 4 groups of one row (V - masked = 79 > K: an unpenalised word always exists): no two live hypotheses take the
    same word at a step; every image returns K hypotheses; the result differs from the plain beam; distinct-1 and distinct-2 of each
    image's list are >= the plain beam's and strictly greater on BITE_STRICT = 9 of 9 images (established with group_ref and
    history_ref on the CPU; the margins of both are asserted here, so the GPU lists are the CPU's); and fin_score of every hypothesis is,
    within 1e-4, the sum of its words' log-probabilities teacher-forced through group_ref.decode_step: the penalty did not leak."""
    import sat_amd  # noqa: F401
    from sat_amd.metrics import distinct_n
    K, seed = 4, BITE_SEEDS[layers]
    dec, hp, ann = TC._setup(layers, seed=seed)
    sd, _, ann_img = _cpu_inputs(layers, seed)
    END = int(hp.vocab_stoi["<END>"])
    kw = dict(max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True)
    mp, mg = {}, {}
    with torch.no_grad():
        ref_plain = HR.beam_search(sd, hp, ann_img, beamk=K, margins=mp, **kw)
        ref_group = GR.beam_search(sd, hp, ann_img, beamk=K, beam_groups=K, diversity_penalty=1e4, margins=mg, **kw)
    for m in (mp, mg):
        b, _, f, _ = _margins(m)
        assert b >= 1e-3 and f >= 2e-4
    plain = _batched(layers, seed, K)
    got = _batched(layers, seed, K, beam_groups=K, diversity_penalty=1e4)
    assert plain[0] == ref_plain[0] and got[0] == ref_group[0]
    assert all(len(caps) == K for caps in got[0]) and got[0] != plain[0]
    strict = {1: 0, 2: 0}
    for n in (1, 2):
        for b in range(9):
            dg, dp = distinct_n(got[0][b], n), distinct_n(plain[0][b], n)
            assert dg >= dp, (n, b, dg, dp)
            strict[n] += dg > dp
    print("distinct-1 / distinct-2 strictly above the plain beam on %d / %d of 9 images" % (strict[1], strict[2]))
    assert strict[1] >= BITE_STRICT and strict[2] >= BITE_STRICT
    o = {k: v.cpu() for k, v in dec._beam_search_device(ann, K, S, TEMPS, "beam", 3, None, None, None, None, False, beam_groups=K,
                                                        diversity_penalty=1e4).items() if k != "ws"}
    assert o["fin_count"].tolist() == [K] * 9
    worst = 0.0
    for b in range(9):
        steps, fin = _kept_words(o, b, K, END)
        for s, kept in steps.items():
            words = [w for _, w in kept]
            assert len(set(words)) == len(words), (b, s, kept)
        for f in range(K):
            g = int(o["fin_row"][b, f])
            said = [w for s in range(fin[g] + 1) for gg, w in steps[s] if gg == g]
            lp = GR.sequence_logprob(sd, hp, ann_img[b], said, TEMPS)
            err = abs(lp - float(o["fin_score"][b, f])) / max(1.0, abs(lp))
            worst = max(worst, err)
            assert err <= 1e-4, (b, f, lp, float(o["fin_score"][b, f]))
    print("fin_score against the teacher-forced sum of log-probabilities: worst relative error %.2e" % worst)


# ------------------------------------------------------------------------------------------------ 6. combination
@pytest.mark.parametrize("K,G", [(4, 2), (6, 2)])
@pytest.mark.parametrize("layers", [1, 2])
def test_history_rules_and_banned_ids_hold_in_every_group(layers, K, G):
    """6. no_repeat_ngram = 2, min_length = 3, no_unk and two banned ids under G = 2: no returned caption repeats a bigram, none is shorter
    than three words, no banned id appears, every image returns K hypotheses, and the result differs both from the same groups without
    the rules and from the ruled search without groups"""
    from collections import Counter
    seed = REF_SEEDS[layers]
    _, hp, _ = TC._setup(layers, seed=seed)
    special = {int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")}
    unruled = _batched(layers, seed, K, beam_groups=G, diversity_penalty=0.5)
    common = [t for t, _ in Counter(t for caps in unruled[0] for c in caps for t in c if t not in special).most_common(2)]
    rules = dict(no_repeat_ngram=2, min_length=3, no_unk=True, banned=common)
    got = _batched(layers, seed, K, beam_groups=G, diversity_penalty=0.5, **rules)
    assert sum(HR.repeats_ngram(c, 2) for caps in unruled[0] for c in caps) >= 5
    TH._check_properties(got[0], rules)
    assert all(len(caps) == K for caps in got[0])
    ban = set(common) | {int(hp.vocab_stoi["<UNK>"])}
    assert not any(t in ban for caps in got[0] for c in caps for t in c)
    assert got[0] != unruled[0] and got[0] != _batched(layers, seed, K, **rules)[0]
    # the groups of an image are beams of their own: parents stay inside the group at every step
    dec, _, ann = TC._setup(layers, seed=seed)
    o = dec._beam_search_device(ann, K, S, TEMPS, "beam", 3, None, None, None, None, False, beam_groups=G, diversity_penalty=0.5, **rules)
    prev, Kg = o["prev_row"].cpu(), K // G
    rows = torch.arange(K) // Kg
    assert torch.equal(prev[1:] // Kg, rows.expand_as(prev[1:]))
    assert o["fin_count"].cpu().tolist() == [K] * 9 and torch.equal(torch.sort(o["fin_row"].cpu() // Kg, dim=1).values, o["fin_row"].cpu() // Kg)


# ------------------------------------------------------------------------------------------------ 7. surface
def test_evaluation_surface_takes_the_groups():
    """7. val_batch_stats(..., beam_groups=2).metrics() against score_captions on caption(..., beam_groups=2): bleu / gleu exactly, cosine
    within max(2 e_torch, 1e-6) of the float64 value, perplexity 1e-6 relative (the rule of the neighbouring surface tests); and
    sat_beam_select on the merged buffers picks the hypothesis the host back-trace picks"""
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, model as M
    from oracle import prng, sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16,
                decoder_dim=40, deep_output=True, val_beamk=3, val_max_len=7)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over))).cuda()
    img = torch.from_numpy(prng.uniform((4, 3, 64, 64), 41, 0.0, 1.0)).cuda()
    caps, lengths = prng.captions(4, 3, 9, 60, 42, min_len=3)
    caps, lengths = torch.from_numpy(caps).cuda(), torch.from_numpy(lengths)
    kw = dict(beamk=4, max_gen_length=7, temperature=1.0, rescore_method="LN", rescore_reward=0.7, beam_groups=2, diversity_penalty=0.5)
    captions, scores, _, ppl = model.caption(img, return_all=False, **kw)
    want = model.score_captions(captions, caps, lengths, ppl)
    assert want == model.val_batch((img, caps, lengths), **kw)
    got = model.val_batch_stats((img, caps, lengths), **kw).metrics()
    assert set(got) == set(want)
    for k in ("bleu1", "bleu2", "bleu3", "bleu4", "gleu"):
        assert got[k] == want[k], (k, got[k], want[k])
    E64 = model.embedding.weight.detach().cpu().double()
    c64 = []
    for i, h in enumerate(captions):
        cv = E64[torch.as_tensor(h, dtype=torch.long)].mean(0)
        rvs = [E64[caps[i][j][1:int(l)].cpu()].mean(0) for j, l in enumerate(lengths[i])]
        c64.append(max(float(((rv / rv.norm().clamp_min(1e-8)) * (cv / cv.norm().clamp_min(1e-8))).sum()) for rv in rvs))
    c64 = sum(c64) / len(c64)
    e_kernel, e_torch = abs(got["cosine_similarity"] - c64), abs(want["cosine_similarity"] - c64)
    print("cosine: e_kernel %.3e  e_torch %.3e" % (e_kernel, e_torch))
    assert e_kernel <= max(2 * e_torch, 1e-6)
    assert abs(got["perplexity"] - want["perplexity"]) <= 1e-6 * abs(want["perplexity"])
    # sat_beam_select (caption_tokens) on the merged buffers against the host back-trace of caption()
    tok, ln, sc, pp = model.caption_tokens(img, **kw)
    tok, ln = tok.cpu().tolist(), ln.cpu().tolist()
    for b in range(4):
        assert tok[b][:ln[b]] == captions[b] and tok[b][ln[b]:] == [model.pad_idx] * (8 - ln[b]), b
        assert abs(float(sc[b]) - scores[b]) <= 1e-6 * max(1.0, abs(scores[b])) and abs(float(pp[b]) - ppl[b]) <= 1e-6 * ppl[b]
    words = model.caption_image([np.zeros((80, 80, 3), np.uint8)], beamk=4, max_gen_length=7, rescore_method="LN", beam_groups=2)
    assert len(words[0]) == 1


@pytest.mark.parametrize("layers", [1, 2])
def test_mbr_votes_over_a_grouped_beam(layers):
    """7. rescore_method="MBR" over a grouped beam runs and returns K utilities per image, each the host's metrics.consensus_utilities of
    the grouped beam's own list within the bound of tests/test_gpu_mbr.py"""
    import test_gpu_mbr as TM
    import mbr_cases as MC
    m = TM._metrics()
    K, seed = 6, REF_SEEDS[layers]
    dec, hp, ann = TC._setup(layers, seed=seed)
    rc, df, n_images = TM._e2e_corpus()
    kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, beam_groups=3, diversity_penalty=0.5, return_all=True)
    base = dec.beam_decode_batched(ann, HW, rescore_method=None, **kw)
    reward, alpha = (0.5, 0.5), 1.0
    every = dec.beam_decode_batched(ann, HW, rescore_method="MBR", mbr_corpus=rc, mbr_reward=reward, mbr_alpha=alpha, **kw)
    for b in range(9):
        assert len(every[1][b]) == K and len(every[0][b]) == K
        host = m.consensus_utilities(base[0][b], base[1][b], df, n_images, reward, alpha)
        assert sorted(map(tuple, every[0][b])) == sorted(map(tuple, base[0][b]))
        for u, v in zip(sorted(every[1][b]), sorted(host)):
            assert abs(u - v) <= MC.bound(reward, v), (b, u, v)
        assert all(every[1][b][i] >= every[1][b][i + 1] for i in range(K - 1))
