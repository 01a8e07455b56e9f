"""CPU: required words of the batched caption search ("Required words").  Every refusal of the Python surface and of the C
entry points before anything is launched, the CPU reference (tests/required_ref.py) against tests/history_ref.py where the two must
agree and its own guarantees, and constraints.required_coverage on hand-written captions."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import history_ref as HR
import required_ref as RR

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


def _stoi():
    stoi = {"<START>": 0, "<PAD>": 1, "<END>": 2, "<UNK>": 3}
    stoi.update({w: 4 + i for i, w in enumerate("a dog cat frisbee grass on the runs".split())})
    return stoi


def test_resolve_required_raises_every_value_error():
    """1. the "off" spellings return None; the accepted forms; every refusal names its argument"""
    import sat_amd  # noqa: F401
    from sat_amd import constraints as Cn
    stoi = _stoi()

    def r(required, B=3, beamk=K, S_=S, **kw):
        return Cn.resolve_required(stoi, V, B, beamk, S_, required, **kw)
    for off in (None, [], "", "   ", [[], [], []], ["", [], ""], torch.zeros(0, dtype=torch.int64)):
        assert r(off) is None
    assert r(None, sample_method="topk", topg=3, prefix=[5], graph=True, batched=False) is None     # off: nothing is checked
    assert r([], beamk=1000, decoder_noise=0.5) is None
    assert r("dog frisbee").words == [[5, 7]] * 3 and r([5, 7]).words == [[5, 7]] * 3 and r(torch.tensor([5, 7])).words == [[5, 7]] * 3
    got = r(["dog", [], [7, 6, 4]])
    assert got.words == [[5], [], [7, 6, 4]] and got.max_required == 3
    assert r([["dog", "cat"], "grass", []]).words == [[5, 6], [8], []]
    st, keep = got.device_struct("cpu")
    assert st.max_required == 3 and C.sizeof(st) == 24 and keep[0].tolist() == [[5, 0, 0], [0, 0, 0], [7, 6, 4]] and keep[1].tolist() == [1, 0, 3]
    assert keep[0].dtype == torch.int32 and keep[1].dtype == torch.int32
    bad = [(dict(required="dog zebra"), "zebra"), (dict(required=[5, 83]), "required id 83"), (dict(required=[-1]), "required id -1"),
           (dict(required=[2]), "<END>"), (dict(required="<UNK>"), "<UNK>"), (dict(required=[[0], [], []]), "<START>"), (dict(required=[1]), "<PAD>"),
           (dict(required=[5, 6], banned=[6]), "banned id 6"), (dict(required=[5, 6], banned=torch.tensor([5])), "banned id 5"),
           (dict(required=[5, 6, 5]), "repeat"), (dict(required=[[5], [6, 6], []]), "image 1"),
           (dict(required=list(range(4, 13))), "at most 8"), (dict(required=[4, 5, 6], S_=2), "max_gen_length"),
           (dict(required=[[5], [6]]), "2 word lists for 3 images"), (dict(required=[5], beamk=257), "beamk"),
           (dict(required=[5], sample_method="multinomial"), "sample_method"), (dict(required=[5], sample_method="nucleus"), "sample_method"),
           (dict(required=[5], sample_method="ancestral", beamk=1), "sample_method"), (dict(required=[5], decoder_noise=0.3), "decoder_noise"),
           (dict(required=[5], topg=3), "topg"), (dict(required=[5], prefix="a dog"), "prefix"), (dict(required=[5], beam_groups=2), "beam_groups"),
           (dict(required=[5], graph=True), "graph"), (dict(required=[5], batched=False), "beam_decode"), (dict(required=[5], S_=128), "max_gen_length"),
           (dict(required=[5], beamk=71), "unmasked ids left"), (dict(required=[5], beamk=68, banned=[9, 10, 11]), "unmasked ids left")]
    for kw, word in bad:
        with pytest.raises(ValueError, match=re.escape(word)):
            r(**kw)
    assert r([5], beam_groups=1) is not None and r([5], decoder_noise=0.0) is not None
    assert r([5], beamk=70) is not None                                      # 83 - 4 - 9 = 70 ids are left: beamk 70 fits
    assert r([5, 6], no_unk=True).words == [[5, 6]] * 3


def test_python_surface_raises_before_touching_a_gpu():
    """1. CPU tensors: a call that got past the checks fails with SatHipError (there is no CPU fallback); the Ensemble refuses"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, ensemble as En, evaluation as E, model as M, visualize as Z
    from oracle import sat_oracle as O
    dec, hp = _decoder()
    ann = torch.zeros(3, 12, 32)
    bad = [(dict(required=[5, 5]), "repeat"), (dict(required=[int(hp.vocab_stoi["<END>"])]), "<END>"), (dict(required=[99]), "required id"), (dict(required=[[5]]), "word lists"),
           (dict(required=[5], sample_method="topk"), "sample_method"), (dict(required=[5], sample_method="nucleus", seed=3), "sample_method"),
           (dict(required=[5], decoder_noise=0.2), "decoder_noise"), (dict(required=[5], topg=2), "topg"), (dict(required=[5], prefix=[5, 6]), "prefix"),
           (dict(required=[5], beam_groups=2), "beam_groups"), (dict(required=[5], graph=True), "graph"), (dict(required=[5], banned=[5]), "banned"),
           (dict(required=list(range(10, 19))), "at most 8")]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            dec.beam_decode_batched(ann, (3, 4), beamk=K, max_gen_length=S, **kw)
    with pytest.raises(ValueError, match="max_gen_length"):
        dec.beam_decode_batched(ann, (3, 4), beamk=K, max_gen_length=2, required=[5, 6, 7])
    with pytest.raises(ValueError, match="beam_decode"):                     # the per-image loop has no required words
        dec.beam_decode(ann, (3, 4), beamk=K, max_gen_length=S, required=[5])
    with pytest.raises(L.SatHipError):                                       # "off" reaches the loop's GPU check
        dec.beam_decode(ann, (3, 4), beamk=K, max_gen_length=S, required=[])
    for kw in (dict(required=[5]), dict(required=[[5, 6], [], [7]]), dict(required=[5, 6], no_repeat_ngram=2, no_unk=True, banned=[7]),
               dict(required=None), dict(required=[[], [], []])):
        with pytest.raises(L.SatHipError):                                   # well-formed words reach the GPU check
            dec.beam_decode_batched(ann, (3, 4), beamk=K, max_gen_length=S, **kw)
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over)))
    img = torch.zeros(2, 3, 64, 64)
    caps, lens = torch.zeros(2, 3, 9, dtype=torch.int64), torch.full((2, 3), 4)
    pic = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(ValueError, match="required id"):
        model.caption(img, beamk=3, required=[60])
    with pytest.raises(ValueError, match="beam_decode"):
        model.caption(img, beamk=4, max_gen_length=0, required=[9])
    with pytest.raises(ValueError, match="topg"):
        model.forward(img, beamk=4, required=[9], topg=2)
    with pytest.raises(ValueError, match="sample_method"):
        E.caption_tokens(model, img, beamk=4, sample_method="multinomial", required=[9])
    with pytest.raises(ValueError, match="graph"):
        model.caption_tokens(img, beamk=4, graph=True, required=[9])
    with pytest.raises(ValueError, match="repeat"):
        model.val_batch_stats((img, caps, lens), beamk=4, required=[[9, 9], []])
    with pytest.raises(ValueError, match="prefix"):
        Z.caption_image(model, pic, beamk=4, required=[9], prefix=[9])
    with pytest.raises(ValueError, match="beam_groups"):
        model.visualize(pic, beamk=4, beam_groups=2, required=[9])
    with pytest.raises(ValueError, match="word lists"):
        model.caption_image(pic, beamk=4, required=[[9], [10]])
    ens = En.Ensemble([model, model])
    with pytest.raises(ValueError, match="required"):
        ens.caption(img, beamk=3, required=[9])
    with pytest.raises(ValueError, match="required"):
        En.Ensemble([model]).caption(img, beamk=3, required="x")
    model.beam_graph = True
    with pytest.raises(ValueError, match="graph"):
        model.caption(img, beamk=4, required=[9])


def test_header_and_library_declare_the_required_entry_points():
    """three new symbols, two limits and a struct of 24 bytes; the version stays 23"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, constraints as Cn
    text = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    assert "#define SAT_HIP_ABI_VERSION 23" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sat_beam_search_required_workspace_bytes", "sat_beam_search_required", "sat_beam_required_select"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.SYMBOLS
    assert re.search(r"#define SAT_BEAM_REQUIRED_MAX\s+%d\b" % Cn.REQUIRED_MAX, code) and Cn.REQUIRED_MAX == 8
    assert re.search(r"#define SAT_BEAM_REQUIRED_MAX_K\s+%d\b" % Cn.REQUIRED_MAX_BEAMK, code) and Cn.REQUIRED_MAX_BEAMK == 256
    assert re.search(r"typedef struct sat_beam_required \{[^}]*int32_t max_required;[^}]*int32_t reserved;[^}]*const int32_t\* words;[^}]*"
                     r"const int32_t\* n_words;[^}]*\} sat_beam_required;", code)
    assert C.sizeof(L.BeamRequired) == 24
    assert L.lib().sat_abi_version() == 23


def _call_search(dec, hp, req, con=None, smp=None, hist=None, beamk=K, B=2, S_=S, req_met=True):
    """sat_beam_search_required on host pointers: every check under test runs before the first launch, nothing is dereferenced"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    dims = Dk.decoder_dims(B, beamk, 2, 12, 32, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    w, keep = dec._params_struct()
    p = torch.zeros(64, dtype=torch.int32).data_ptr()
    temps = (C.c_float * 1)(1.0)
    ids = (C.c_int32 * 4)(*[int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    rc = lib.sat_beam_search_required(C.byref(dims), C.byref(w), p, beamk, S_, temps, 1, ids, C.byref(smp) if smp is not None else None,
                                      C.byref(con) if con is not None else None, C.byref(hist) if hist is not None else None,
                                      C.byref(req) if req is not None else None, p, p, p, p, p, p, p, p, p if req_met else None, p, 1 << 40, None)
    return rc, lib.sat_last_error().decode()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """2. SAT_EINVAL with a message naming the argument; the pointers are never followed; the workspace query refuses the same sizes"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, decoder as Dk
    dec, hp = _decoder()
    p = torch.zeros(64, dtype=torch.int32).data_ptr()

    def R(c=2, words=p, n_words=p):
        return L.BeamRequired(max_required=c, words=words, n_words=n_words)
    cases = [(dict(req=R(-1)), "max_required -1 outside 0..8"), (dict(req=R(9)), "max_required 9 outside 0..8"),
             (dict(req=R(2, words=None)), "null pointer (words / n_words"), (dict(req=R(2, n_words=None)), "null pointer (words / n_words"),
             (dict(req=R(2), req_met=False), "null pointer (req_met"), (dict(req=R(2), beamk=257), "beamk 257 above 256"),
             (dict(req=R(3), S_=2), "max_required 3 above max_gen_length 2"), (dict(req=R(2), S_=128), "max_gen_length 128 is over the limit"),
             (dict(req=R(2), smp=L.BeamSampling(method=1, seed=1)), "sampling"), (dict(req=R(2), smp=L.BeamSampling(method=2, sample_topk=3, seed=1)), "sampling"),
             (dict(req=R(2), smp=L.BeamSampling(method=3, sample_topp=0.9, seed=1)), "sampling"),
             (dict(req=R(2), smp=L.BeamSampling(method=4, seed=1), beamk=1), "sampling"),
             (dict(req=R(2), smp=L.BeamSampling(method=0, decoder_noise=0.5, seed=1)), "decoder_noise"),
             (dict(req=R(2), con=L.BeamConstraints(topg=2)), "topg"),
             (dict(req=R(2), con=L.BeamConstraints(max_prefix=2, prefix=p, prefix_len=p)), "prefix"),
             (dict(req=R(2), hist=L.BeamHistory(no_repeat_ngram=-1)), "no_repeat_ngram")]
    for kw, word in cases:
        rc, msg = _call_search(dec, hp, **kw)
        assert rc != 0 and "beam_" in msg and word in msg, (word, rc, msg)
    # the workspace query: the history figure at topg = 0, and the refusals of the search
    lib = L.lib()
    dims = Dk.decoder_dims(2, K, 2, 12, 32, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    base = lib.sat_beam_search_history_workspace_bytes(C.byref(dims), K, 0, S)
    q = lib.sat_beam_search_required_workspace_bytes
    assert q(C.byref(dims), K, S, 0) == base and q(C.byref(dims), K, S, 1) == base and q(C.byref(dims), K, S, 8) == base
    for args, word in (((K, S, -1), "max_required"), ((K, S, 9), "max_required"), ((257, S, 2), "beamk"), ((K, 2, 3), "max_gen_length"),
                       ((K, 128, 2), "max_gen_length"), ((K, -1, 0), "max_gen_length")):
        assert q(C.byref(dims), *args) == 0 and word in lib.sat_last_error().decode(), args
    assert q(C.byref(dims), K, 300, 0) > 0 and q(C.byref(dims), 300, S, 0) > 0          # off: a long or wide search is served

    # sat_beam_required_select
    def select(B=2, beamk=6, v=V, stride=10, hist=p, req=R(3), scores=p, klive=p, work=p, values=p, indices=p):
        rc = lib.sat_beam_required_select(scores, klive, B, beamk, v, hist, stride, 3, 0, C.byref(req) if req is not None else None, 2, work, values,
                                          indices, None)
        return rc, lib.sat_last_error().decode()
    bad = [(dict(B=0), "size"), (dict(beamk=0), "size"), (dict(v=0), "size"), (dict(beamk=257), "256"), (dict(req=R(9)), "max_required"),
           (dict(req=R(-2)), "max_required"), (dict(stride=-1), "hist_stride"), (dict(stride=129), "hist_stride"), (dict(hist=None), "null pointer"),
           (dict(req=R(2, words=None)), "null pointer"), (dict(req=R(2, n_words=None)), "null pointer"), (dict(req=None), "null pointer"),
           (dict(scores=None), "null pointer"), (dict(klive=None), "null pointer"), (dict(work=None), "null pointer"),
           (dict(values=None), "null pointer"), (dict(indices=None), "null pointer")]
    for kw, word in bad:
        rc, msg = select(**kw)
        assert rc != 0 and "beam_required_select" in msg and word in msg, (word, rc, msg)


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
def test_reference_without_words_is_the_history_reference(layers):
    """3. no required words (None, or an empty list per image) is history_ref.beam_search float for float, without and with the rules"""
    sd, hp, ann = _reference_inputs(layers)
    for rules in (dict(), dict(no_repeat_ngram=2, min_length=3, repetition_penalty=1.3)):
        kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="BAR", return_all=True, **rules)
        with torch.no_grad():
            want = HR.beam_search(sd, hp, ann, **kw)
            for req in (None, [[]] * 9):
                info = {}
                _identical(RR.beam_search(sd, hp, ann, required=req, info=info, **kw), want)
                assert info["req_met"] == [0] * 9
    with torch.no_grad():
        _identical(RR.beam_search(sd, hp, ann, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN"),
                   HR.beam_search(sd, hp, ann, beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN"))


def unsaid_words(plain_all, hp, C_, skip=()):
    """per image, the C_ lowest non-special ids that no hypothesis of the plain beam says (``plain_all``: a return_all result)"""
    special = {int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")} | set(skip)
    out = []
    for caps in plain_all[0]:
        said = {t for c in caps for t in c}
        out.append([v for v in range(hp.vocab_size) if v not in said and v not in special][:C_])
    return out


def ruled_banned(result_all, hp, req):
    """<UNK> and the two commonest ordinary words of a return_all result that no image requires (ties: the first met)"""
    from collections import Counter
    skip = {int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")} | {w for r in req for w in r}
    common = [t for t, _ in Counter(t for caps in result_all[0] for c in caps for t in c if t not in skip).most_common(2)]
    return sorted(common + [int(hp.vocab_stoi["<UNK>"])])


@pytest.mark.parametrize("layers,C_", [(1, 1), (1, 3), (2, 2)])
def test_reference_meets_the_words_the_plain_beam_does_not_say(layers, C_):
    """3. words the plain beam never says: every hypothesis that ended in <END> contains them all, req_met == C_b, every kept hypothesis
    reaches it, a mixed batch leaves the images without words alone, and a score is the model's log-probability of its words"""
    import group_ref as GR
    sd, hp, ann = _reference_inputs(layers)
    kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, return_all=True)
    with torch.no_grad():
        plain = HR.beam_search(sd, hp, ann, **kw)
        req = unsaid_words(plain, hp, C_)
        req[4] = []
        if C_ > 1:
            req[7] = req[7][:1]
        info = {}
        got = RR.beam_search(sd, hp, ann, required=req, info=info, **kw)
        assert info["req_met"] == [len(r) for r in req]
        for b in range(9):
            assert len(got[0][b]) >= 1
            assert all(RR.count_required(c, req[b]) == len(req[b]) for c in got[0][b])
            if req[b]:
                assert all(RR.count_required(c, req[b]) == 0 for c in plain[0][b])
            else:
                assert got[0][b] == plain[0][b] and got[1][b] == plain[1][b]
        # before the compaction: whatever ended by saying <END> had said every word
        assert all(n == len(req[b]) for b in range(9) for by_end, n in info["ended"][b] if by_end)
        # max_gen_length == C_b still meets every word by the cut
        short = RR.beam_search(sd, hp, ann, required=req, info=(i2 := {}), **dict(kw, max_gen_length=C_))
        assert i2["req_met"] == [len(r) for r in req] and all(len(c) == C_ for b in range(9) if len(req[b]) == C_ for c in short[0][b])
        # a score is the model's log-probability of the words, teacher-forced from the beam's own initial state: nothing of the
        # allocation leaks into it
        for b in (0, 5):
            for said, slot, raw in info["said"][b]:
                assert abs(RR.sequence_logprob(sd, hp, ann[b], said, TEMPS, K, slot) - raw) <= 1e-4
        w = info["said"][0][0][0]
        assert RR.sequence_logprob(sd, hp, ann[0], w, TEMPS) == GR.sequence_logprob(sd, hp, ann[0], w, TEMPS)


def test_select_restates_the_contract_on_a_hand_made_step():
    """the numpy selection on a step small enough to do by hand: V = 6, END = 2, two rows, words {4, 5}"""
    NEG = -np.inf
    x = np.array([[[-1.0, -9.0, -0.5, -3.0, -7.0, -8.0],          # row 0 has said 4: bank 1; its best word is END (held back: 5 is missing)
                   [-2.0, -9.5, NEG, -2.5, -6.0, NEG]]], np.float32)   # row 1 has said nothing; word 5 is at -inf for it
    hist = np.array([[4, 0], [3, 0]])
    v, i = RR.select(x, [2], hist, 1, [[4, 5]], [2], False, 2)
    # A = {(0,0), (1,0)}; R = {(0,5), (1,4)}; M = {(0,0), (1,0)}.  banks: (0,5) -> 2, (0,0) -> 1, (1,4) -> 1, (1,0) -> 0
    # pick 0 from bank 2: (0,5); p = 1: pick 1 from bank 1: (0,0) at -1.0 beats (1,4) at -6.0
    assert i.tolist() == [[5, 0]] and v.tolist() == [[-8.0, -1.0]]
    v, i = RR.select(x, [2], np.array([[4, 5], [3, 0]]), 2, [[4, 5]], [2], False, 2)         # row 0 has said both: END is free
    # row 0 is complete, so (0,2) = END and (0,0) are both bank 2; pick 0 takes END, then p = 1 and bank 1 holds (1,4) alone: the round
    # robin gives the second slot to the hypothesis that gains a word, not to the better (0,0)
    assert i.tolist() == [[2, 10]] and v.tolist() == [[-0.5, -6.0]]
    # the same step as the last one of a search (first & 2): the word picked now is not part of the caption, so (1,4) counts as bank 0 and
    # loses its slot to nobody in bank 1; the walk from p = 1 reaches bank 0 and takes its best, (1,0) at -2.0
    v, i = RR.select(x, [2], np.array([[4, 5], [3, 0]]), 2, [[4, 5]], [2], 2, 2)
    assert i.tolist() == [[2, 6]] and v.tolist() == [[-0.5, -2.0]]


def test_required_coverage_on_hand_written_captions():
    """4. the fraction of an image's required words its caption says; strings, word lists and ids; shared and per image"""
    import sat_amd  # noqa: F401
    from sat_amd.constraints import required_coverage as cov
    caps = [["a", "dog", "catches", "a", "frisbee"], ["a", "cat"], []]
    assert cov(caps, "dog frisbee") == [1.0, 0.0, 0.0]
    assert cov(caps, ["dog frisbee", "cat dog", ""]) == [1.0, 0.5, 1.0]
    assert cov(caps, [["frisbee", "grass", "dog"], [], ["x"]]) == [2 / 3, 1.0, 0.0]
    assert cov(caps, None) == [1.0, 1.0, 1.0] and cov([], None) == []
    assert cov(["a dog on grass", "the cat"], "dog cat") == [0.5, 0.5]
    assert cov([[4, 5, 9], [6]], [5, 6]) == [0.5, 0.5] and cov([[4, 5, 9], [6]], [[9, 4], [7]]) == [1.0, 0.0]
    assert cov([torch.tensor([4, 5, 9])], torch.tensor([5, 7])) == [0.5]
    stoi = _stoi()
    assert cov([[4, 5, 9], ["a", "cat"]], "dog cat", stoi) == [0.5, 0.5]            # ids against words through the vocabulary
    assert cov([["a", "zebra"]], [[3]], stoi) == [1.0]                                 # a word outside the vocabulary is <UNK>
    with pytest.raises(ValueError, match="word lists"):
        cov(caps, [["dog"]])
