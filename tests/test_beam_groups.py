"""CPU: the diverse (group) beam search ("Diverse beam search").  Every refusal of the Python surface and of the C entry
points before anything is launched, the CPU reference (tests/group_ref.py) against tests/history_ref.py where the two must agree,
and metrics.distinct_n on hand-made lists."""
import ctypes as C
import os
import re

import pytest
import torch

import group_ref as GR
import history_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K, S = 83, 4, 9
TEMPS = [1.0, 0.7]


def _decoder(layers=1, seed=None):
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    hp = O.default_hparams(vocab_size=V, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40, decoder_layers=layers)
    torch.manual_seed(3 + layers if seed is None else seed)
    return M.SATDecoder(hp).eval(), hp


def test_resolve_groups_raises_every_value_error():
    """1. the "off" spellings return None whatever the penalty says; every refusal names its argument"""
    import sat_amd  # noqa: F401
    from sat_amd import constraints as Cn
    r = Cn.resolve_groups
    for kw in (dict(), dict(beam_groups=None), dict(beam_groups=0), dict(beam_groups=1), dict(beam_groups=1, diversity_penalty=-3.0),
               dict(beam_groups=None, diversity_penalty=float("nan")), dict(beam_groups=1, sample_method="nucleus", topg=2, prefix=[5], graph=True)):
        assert r(K, **kw) is None
    assert r(K, 1, batched=False) is None
    got = r(6, 3, 0.25, V=V)
    assert (got.groups, got.diversity_penalty) == (3, 0.25)
    st = got.device_struct()
    assert (st.groups, st.diversity_penalty) == (3, 0.25) and C.sizeof(st) == 8
    assert r(K, K, 0.0).diversity_penalty == 0.0 and r(K, 2).diversity_penalty == 0.5
    bad = [(dict(beam_groups=-1), "beam_groups"), (dict(beam_groups=3), "beam_groups"), (dict(beam_groups=8), "beam_groups"),
           (dict(beam_groups=2, diversity_penalty=-0.1), "diversity_penalty"), (dict(beam_groups=2, diversity_penalty=float("inf")), "diversity_penalty"),
           (dict(beam_groups=2, diversity_penalty=float("nan")), "diversity_penalty"), (dict(beam_groups=2, diversity_penalty="much"), "diversity_penalty"),
           (dict(beam_groups=2, sample_method="multinomial"), "sample_method"), (dict(beam_groups=2, sample_method="topk"), "sample_method"),
           (dict(beam_groups=2, sample_method="nucleus"), "sample_method"), (dict(beam_groups=2, decoder_noise=0.3), "decoder_noise"),
           (dict(beam_groups=2, topg=3), "topg"), (dict(beam_groups=2, prefix="a photo"), "prefix"), (dict(beam_groups=2, prefix=[[5]] * 3), "prefix"),
           (dict(beam_groups=2, graph=True), "graph"), (dict(beam_groups=2, batched=False), "beam_decode")]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            r(K, **kw)
    with pytest.raises(ValueError, match="1024"):
        r(2048, 2)
    with pytest.raises(ValueError, match="V="):
        r(8, 2, V=3)
    assert r(K, 2, decoder_noise=0.0) is not None and r(K, 2, decoder_noise=None) is not None


def test_python_surface_raises_before_touching_a_gpu():
    """1. CPU tensors: a call that got past the checks fails with SatHipError (there is no CPU fallback)"""
    import numpy as np
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, evaluation as E, model as M, visualize as Z
    from oracle import sat_oracle as O
    dec, hp = _decoder()
    ann = torch.zeros(3, 12, 32)
    bad = [(dict(beam_groups=3), "beam_groups"), (dict(beam_groups=-2), "beam_groups"), (dict(beam_groups=2, diversity_penalty=-1.0), "diversity_penalty"),
           (dict(beam_groups=2, sample_method="topk"), "sample_method"), (dict(beam_groups=2, sample_method="nucleus", seed=3), "sample_method"),
           (dict(beam_groups=2, decoder_noise=0.2), "decoder_noise"), (dict(beam_groups=2, topg=2), "topg"), (dict(beam_groups=2, prefix=[5, 6]), "prefix"),
           (dict(beam_groups=2, graph=True), "graph")]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            dec.beam_decode_batched(ann, (3, 4), beamk=K, max_gen_length=S, **kw)
    with pytest.raises(ValueError, match="ancestral|sample_method"):
        dec.beam_decode_batched(ann, (3, 4), beamk=1, max_gen_length=S, sample_method="ancestral", beam_groups=2)
    with pytest.raises(ValueError, match="beam_decode"):                     # the per-image loop has no groups
        dec.beam_decode(ann, (3, 4), beamk=K, max_gen_length=S, beam_groups=2)
    with pytest.raises(L.SatHipError):                                       # groups "off" reach the loop's GPU check
        dec.beam_decode(ann, (3, 4), beamk=K, max_gen_length=S, beam_groups=1)
    for kw in (dict(beam_groups=2), dict(beam_groups=4, diversity_penalty=0.0), dict(beam_groups=2, no_repeat_ngram=2, no_unk=True, banned=[7]),
               dict(beam_groups=1, diversity_penalty=3.0), dict(beam_groups=None)):
        with pytest.raises(L.SatHipError):                                   # well-formed groups reach the GPU check
            dec.beam_decode_batched(ann, (3, 4), beamk=K, max_gen_length=S, **kw)
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over)))
    img = torch.zeros(2, 3, 64, 64)
    caps, lens = torch.zeros(2, 3, 9, dtype=torch.int64), torch.full((2, 3), 4)
    pic = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(ValueError, match="beam_groups"):
        model.caption(img, beamk=3, beam_groups=2)
    with pytest.raises(ValueError, match="beam_decode"):
        model.caption(img, beamk=4, max_gen_length=0, beam_groups=2)
    with pytest.raises(ValueError, match="topg"):
        model.val_batch((img, caps, lens), beamk=4, beam_groups=2, topg=2)
    with pytest.raises(ValueError, match="sample_method"):
        E.caption_tokens(model, img, beamk=4, sample_method="multinomial", beam_groups=2)
    with pytest.raises(ValueError, match="graph"):
        model.caption_tokens(img, beamk=4, graph=True, beam_groups=2)
    with pytest.raises(ValueError, match="diversity_penalty"):
        model.val_batch_stats((img, caps, lens), beamk=4, beam_groups=2, diversity_penalty=float("inf"))
    with pytest.raises(ValueError, match="decoder_noise"):
        E.evaluate(model, [(img, caps, lens)], beamk=4, beam_groups=4, decoder_noise=0.1)
    with pytest.raises(ValueError, match="prefix"):
        Z.caption_image(model, pic, beamk=4, beam_groups=2, prefix=[9])
    with pytest.raises(ValueError, match="beam_groups"):
        model.visualize(pic, beamk=5, beam_groups=2)
    model.beam_graph = True
    with pytest.raises(ValueError, match="graph"):
        model.caption(img, beamk=4, beam_groups=2)


def test_header_and_library_declare_the_group_entry_points():
    """three new symbols and a struct of two words; the version stays 23"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    assert "#define SAT_HIP_ABI_VERSION 23" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sat_beam_search_groups_workspace_bytes", "sat_beam_search_groups", "sat_beam_group_select"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.SYMBOLS
    assert re.search(r"typedef struct sat_beam_groups \{[^}]*int32_t groups;[^}]*float\s+diversity_penalty;[^}]*\} sat_beam_groups;", code)
    assert C.sizeof(L.BeamGroups) == 8
    assert L.lib().sat_abi_version() == 23


def _call_search(dec, hp, grp, con=None, smp=None, hist=None, beamk=K, B=2):
    """sat_beam_search_groups on host pointers: every check under test runs before the first launch, nothing is dereferenced"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    dims = Dk.decoder_dims(B, beamk, 2, 12, 32, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    w, keep = dec._params_struct()
    ws_bytes = lib.sat_beam_search_groups_workspace_bytes(C.byref(dims), beamk, 1, S)
    p = torch.zeros(64, dtype=torch.int32).data_ptr()
    temps = (C.c_float * 1)(1.0)
    ids = (C.c_int32 * 4)(*[int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    rc = lib.sat_beam_search_groups(C.byref(dims), C.byref(w), p, beamk, S, temps, 1, ids, C.byref(smp) if smp is not None else None,
                                    C.byref(con) if con is not None else None, C.byref(hist) if hist is not None else None,
                                    C.byref(grp) if grp is not None else None, p, p, p, p, p, p, p, p, p, 1 << 40, None)
    return rc, lib.sat_last_error().decode()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """1. SAT_EINVAL with a message naming the argument; the pointers are never followed"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, decoder as Dk
    dec, hp = _decoder()
    G = L.BeamGroups
    p = torch.zeros(64, dtype=torch.int32).data_ptr()
    cases = [(dict(grp=G(groups=-1)), "groups"), (dict(grp=G(groups=3, diversity_penalty=0.5)), "multiple"),
             (dict(grp=G(groups=2, diversity_penalty=-0.5)), "diversity_penalty"), (dict(grp=G(groups=2, diversity_penalty=float("inf"))), "diversity_penalty"),
             (dict(grp=G(groups=2, diversity_penalty=float("nan"))), "diversity_penalty"), (dict(grp=G(groups=1, diversity_penalty=-1.0)), "diversity_penalty"),
             (dict(grp=G(groups=2), smp=L.BeamSampling(method=1, seed=1)), "sampling"), (dict(grp=G(groups=2), smp=L.BeamSampling(method=2, sample_topk=3, seed=1)), "sampling"),
             (dict(grp=G(groups=2), smp=L.BeamSampling(method=3, sample_topp=0.9, seed=1)), "sampling"),
             (dict(grp=G(groups=2), smp=L.BeamSampling(method=0, decoder_noise=0.5, seed=1)), "decoder_noise"),
             (dict(grp=G(groups=2), con=L.BeamConstraints(topg=2)), "topg"),
             (dict(grp=G(groups=2), con=L.BeamConstraints(max_prefix=2, prefix=p, prefix_len=p)), "prefix"),
             (dict(grp=G(groups=2), hist=L.BeamHistory(no_repeat_ngram=-1)), "no_repeat_ngram")]
    for kw, word in cases:
        rc, msg = _call_search(dec, hp, **kw)
        assert rc != 0 and "beam_" in msg and word in msg, (word, rc, msg)
    rc, msg = _call_search(dec, hp, G(groups=2), smp=L.BeamSampling(method=4, seed=1), beamk=2)
    assert rc != 0 and "beam_groups" in msg
    # the workspace query: the history figure at topg = 0 plus, with groups on, the wider live counts and the per-group finished lists
    lib = L.lib()
    dims = Dk.decoder_dims(2, K, 2, 12, 32, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    base = lib.sat_beam_search_history_workspace_bytes(C.byref(dims), K, 0, S)
    q = lib.sat_beam_search_groups_workspace_bytes
    assert q(C.byref(dims), K, 0, S) == base and q(C.byref(dims), K, 1, S) == base
    assert base + (2 * 2 + 4 * 2 * K) * 4 <= q(C.byref(dims), K, 2, S) <= base + 6 * 256 + (2 * 2 + 4 * 2 * K) * 4
    assert q(C.byref(dims), K, 3, S) == 0 and "groups" in lib.sat_last_error().decode()
    assert q(C.byref(dims), K, -1, S) == 0 and "groups" in lib.sat_last_error().decode()
    assert q(C.byref(dims), K, 2, -1) == 0 and "max_gen_length" in lib.sat_last_error().decode()
    assert q(C.byref(dims), K, 2, 300) > 0                                   # a long search without a history rule

    # sat_beam_group_select
    def select(B=2, beamk=6, groups=3, v=V, lam=0.5, scores=p, klive=p, work=p, values=p, indices=p):
        rc = lib.sat_beam_group_select(scores, klive, B, beamk, groups, v, 0, lam, work, values, indices, None)
        return rc, lib.sat_last_error().decode()
    bad = [(dict(B=0), "sizes"), (dict(beamk=0), "sizes"), (dict(groups=0), "sizes"), (dict(v=0), "sizes"), (dict(groups=4), "groups"),
           (dict(beamk=2048, groups=2), "1024"), (dict(beamk=8, groups=2, v=3), "V="), (dict(lam=-1.0), "diversity_penalty"),
           (dict(lam=float("nan")), "diversity_penalty"), (dict(lam=float("inf")), "diversity_penalty"), (dict(scores=None), "null pointer"),
           (dict(klive=None), "null pointer"), (dict(work=None), "null pointer"), (dict(values=None), "null pointer"), (dict(indices=None), "null pointer")]
    for kw, word in bad:
        rc, msg = select(**kw)
        assert rc != 0 and "beam_group_select" in msg and word in msg, (word, rc, msg)


def _reference_inputs(layers, seed=None):
    from oracle import prng
    dec, hp = _decoder(layers, seed)
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    ann = torch.from_numpy(prng.uniform((9, 12, 32), 55, 0.0, 1.0)).reshape(9, 3, 4, 32).permute(0, 3, 1, 2).contiguous()
    return sd, hp, ann


def _identical(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3]
    assert all(torch.equal(u, v) for x, y in zip(a[2], b[2]) for u, v in zip(x, y))


@pytest.mark.parametrize("layers", [1, 2])
def test_reference_with_one_group_is_the_history_reference(layers):
    """2. G = 1 (whatever lambda says) is history_ref.beam_search float for float, without and with the history rules"""
    sd, hp, ann = _reference_inputs(layers)
    for rules in (dict(), dict(no_repeat_ngram=2, min_length=3, repetition_penalty=1.3)):
        kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="BAR", return_all=True, **rules)
        with torch.no_grad():
            want = HR.beam_search(sd, hp, ann, **kw)
            for lam in (0.0, 0.5, 1e4):
                _identical(GR.beam_search(sd, hp, ann, beam_groups=1, diversity_penalty=lam, **kw), want)
    with torch.no_grad():
        best = GR.beam_search(sd, hp, ann, beamk=K, beam_groups=1, max_gen_length=S, temperature=TEMPS, rescore_method="LN")
        _identical(best, HR.beam_search(sd, hp, ann, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN"))


@pytest.mark.parametrize("K_,G", [(4, 2), (4, 4), (6, 3), (6, 2)])
def test_reference_without_penalty_is_independent_small_beams(K_, G):
    """3. lambda = 0: every group is history_ref.beam_search at beamk = K / G, so an image's list holds G copies of that search's list;
    with return_all the sort puts equal scores next to each other"""
    sd, hp, ann = _reference_inputs(1)
    kw = dict(max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True, no_repeat_ngram=3)
    trace = []
    with torch.no_grad():
        small = HR.beam_search(sd, hp, ann, beamk=K_ // G, **kw)
        got = GR.beam_search(sd, hp, ann, beamk=K_, beam_groups=G, diversity_penalty=0.0, trace=trace, **kw)
    for b in range(9):
        assert got[0][b] == [c for c in small[0][b] for _ in range(G)]
        assert got[1][b] == [s for s in small[1][b] for _ in range(G)] and got[3][b] == [p for p in small[3][b] for _ in range(G)]
        assert all(torch.equal(got[2][b][i], small[2][b][i // G]) for i in range(K_))
    # every group of an image kept the same words at every step
    for b, step in {(b, s) for b, s, _, _ in trace}:
        kept = [w for bb, ss, _, w in trace if (bb, ss) == (b, step)]
        assert all(w == kept[0] for w in kept)


def test_reference_penalty_steers_the_selection_only():
    """lambda = 1e4 with one row per group: no word is kept twice at a step, the lists differ from the plain beam's, and every score is
    the sum of the model's log-probabilities of its words (teacher forcing through decode_step), END included"""
    sd, hp, ann = _reference_inputs(1)
    END = int(hp.vocab_stoi["<END>"])
    kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, return_all=True)
    trace = []
    with torch.no_grad():
        plain = HR.beam_search(sd, hp, ann, **kw)
        got = GR.beam_search(sd, hp, ann, beam_groups=K, diversity_penalty=1e4, trace=trace, **kw)
        assert got[0] != plain[0] and all(len(c) == K for c in got[0])
        for b, step in {(b, s) for b, s, _, _ in trace}:
            words = [w for bb, ss, _, kept in trace if (bb, ss) == (b, step) for w in kept]
            assert len(set(words)) == len(words), (b, step, words)
        for b in range(9):
            # one row per group: the words a group kept, step after step, are its hypothesis, the closing <END> or the cut word included
            said = [[kept[0] for bb, _, gg, kept in trace if (bb, gg) == (b, g)] for g in range(K)]
            assert sorted(w[:-1] for w in said) == sorted(got[0][b]) and all(w[-1] == END or len(w) == S + 1 for w in said)
            want = sorted((GR.sequence_logprob(sd, hp, ann[b], w, TEMPS) for w in said), reverse=True)
            assert all(abs(u - v) <= 1e-4 * max(1.0, abs(u)) for u, v in zip(want, got[1][b]))


def test_distinct_n_on_hand_made_lists():
    """4. distinct n-grams over n-grams, pooled over the list"""
    import sat_amd  # noqa: F401
    from sat_amd.metrics import distinct_n
    a = [1, 2, 3, 4]
    assert distinct_n([a], 1) == 1.0 and distinct_n([a], 2) == 1.0 and distinct_n([a], 4) == 1.0
    assert distinct_n([a] * 5, 1) == 1 / 5 and distinct_n([a] * 5, 2) == 1 / 5
    assert distinct_n([[1, 2, 3], [1, 2, 4]], 1) == 4 / 6 and distinct_n([[1, 2, 3], [1, 2, 4]], 2) == 3 / 4
    assert distinct_n([[7, 7, 7, 7]], 1) == 1 / 4 and distinct_n([[7, 7, 7, 7]], 2) == 1 / 3
    assert distinct_n([["a", "dog"], ["a", "cat"], ["the", "dog"]], 1) == 4 / 6
    assert distinct_n([[1, 2], [3]], 2) == 1.0                               # the one-word caption has no bigram
    assert distinct_n([], 1) == 0.0 and distinct_n([[1], [2]], 2) == 0.0 and distinct_n([[]], 1) == 0.0
    assert distinct_n([(1, 2), (2, 1)], 2) == 1.0 and distinct_n([(1, 2), (2, 1)], 1) == 0.5
    with pytest.raises(ValueError):
        distinct_n([a], 0)
