"""CPU: one search descriptor ("One search descriptor").  sat_beam_search and its workspace query on host pointers (every
check under test runs before the first launch, nothing is dereferenced): the declarations, the refusals of the entry points from before
the descriptor reproduced word for word, the refusals only a descriptor can express, the query against the search and against the old
queries; and ``constraints.SearchOptions``, the one refusal sequence of the Python surface."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import pytest
import torch

import beam_search_desc_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K, S = 83, 4, 6


def _decoder(seed=4, **over):
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    hp = O.default_hparams(**dict(dict(vocab_size=V, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40), **over))
    torch.manual_seed(seed)
    return M.SATDecoder(hp).eval(), hp


_P = torch.zeros(64, dtype=torch.int32)          # where every "device" pointer of this file points: never followed
P = _P.data_ptr()
OUTS = (P,) * 8
BIG = 1 << 40


def _single(B=2, Lc=12, beamk=K, S_=S, seed=4, **over):
    """the parts of a single-model search over ``B`` images"""
    from sat_amd import decoder as Dk
    dec, hp = _decoder(seed, **over)
    dims = Dk.decoder_dims(B, beamk, 2, Lc, int(hp.encoder_dim), 16, 24, int(hp.decoder_dim), V, 0, hp.deep_output, dec.pad_idx, 0, layers=int(hp.decoder_layers))
    w, tens = dec._params_struct()
    return BC.Parts(dims=dims, w=w, ann=P, beamk=beamk, S=S_, keep=(dec, tens))


def _ensemble(beamk=K, S_=S, weights=(0.5, 0.5), combine=1):
    """the parts of a search over two members with different L, D, n and layer count"""
    from sat_amd import _lib as L
    a = _single(Lc=12, beamk=beamk, S_=S_)
    b = _single(Lc=6, beamk=beamk, S_=S_, seed=5, encoder_dim=48, decoder_dim=56, decoder_layers=2)
    ens = L.BeamEnsemble(members=2, combine=combine)
    for i, (m, wt) in enumerate(zip((a, b), weights)):
        ens.dims[i], ens.params[i], ens.ann[i], ens.weight[i] = C.pointer(m.dims), C.pointer(m.w), P, wt
    return BC.Parts(ens=ens, beamk=beamk, S=S_, keep=(a, b))


def _tail(msg):
    """a message without the leading name of whoever raised it ("beam_search_history: null pointer" -> "null pointer")"""
    return msg.split(": ", 1)[-1]


def _both(entry, p, outs=OUTS, req_met=P, ws=P, ws_bytes=BIG):
    """((status, message) of the old entry, (status, message) of sat_beam_search) on the same parts"""
    from sat_amd import _lib as L
    lib = L.lib()
    rc_old = BC.old_call(lib, entry, p, outs, req_met, ws, ws_bytes, None)
    msg_old = lib.sat_last_error().decode()
    rc_new = BC.new_call(L, p, outs, req_met, ws, ws_bytes, None)
    return (rc_old, msg_old), (rc_new, lib.sat_last_error().decode())


def _query(p):
    from sat_amd import _lib as L
    n = L.lib().sat_beam_search_desc_workspace_bytes(C.byref(BC.descriptor(L, p)))
    return n, L.lib().sat_last_error().decode()


def test_header_and_binding_declare_the_descriptor():
    """two structs and two functions, in the header and in the ctypes mirror, of the same layout; the version stays 23"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    assert "#define SAT_HIP_ABI_VERSION 23" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sat_beam_search_desc_workspace_bytes", "sat_beam_search"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.SYMBOLS
    desc = re.search(r"typedef struct sat_beam_search_desc \{([^}]*)\} sat_beam_search_desc;", code).group(1)
    out = re.search(r"typedef struct sat_beam_search_out \{([^}]*)\} sat_beam_search_out;", code).group(1)

    def fields(body):
        """[(name, is a pointer)] of a struct body, in declaration order (``T* a;``, ``T *a, *b;`` and ``T a, b;``)"""
        got = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(?:const\s+)?\w+\s*(\**)\s*(.+)", decl)
            for i, name in enumerate(n.strip() for n in m.group(2).split(",")):
                got.append((name.lstrip("* "), name.startswith("*") or (i == 0 and bool(m.group(1)))))
        return got
    for body, mirror in ((desc, L.BeamSearchDesc), (out, L.BeamSearchOut)):
        want = fields(body)
        assert [n for n, _ in want] == [n for n, _ in mirror._fields_]
        for (name, is_ptr), (_, ctype) in zip(want, mirror._fields_):
            assert (C.sizeof(ctype) == 8) == is_ptr and (is_ptr or ctype is C.c_int32), name
    # 4 pointers, 2 ints, a pointer, 2 ints, 6 pointers: no padding on a 64-bit target; nine pointers
    assert C.sizeof(L.BeamSearchDesc) == 11 * 8 + 4 * 4 == 104 and C.sizeof(L.BeamSearchOut) == 9 * 8 == 72
    assert L.BeamSearchDesc.beamk.offset == 32 and L.BeamSearchDesc.temperatures_host.offset == 40 and L.BeamSearchDesc.special_ids_host.offset == 56
    assert L.SEARCH_OUTPUTS[:8] == BC.OUTPUTS and L.SEARCH_OUTPUTS[8] == "req_met"
    assert L.lib().sat_abi_version() == 23


def _refusals():
    """[(old entry, parts, call keywords, a word of the message)]: what the entry points from before the descriptor refuse"""
    from sat_amd import _lib as L
    s = _single()
    Smp, Con, Hist, Grp, Req = L.BeamSampling, L.BeamConstraints, L.BeamHistory, L.BeamGroups, L.BeamRequired
    req2 = Req(max_required=2, words=P, n_words=P)
    cases = [
        # what every entry checks under its own name
        ("batched", s.but(ann=None), {}, "null pointer"), ("batched", s.but(temps=None), {}, "null pointer"), ("sampled", s.but(ids=None), {}, "null pointer"),
        ("history", s, dict(outs=(P, P, None, P, P, P, P, P)), "null pointer"), ("groups", s, dict(ws=None), "null pointer"),
        ("batched", s.but(temps=(1.0, 0.0)), {}, "temperature 0"), ("required", s.but(temps=(-1.0,)), {}, "temperature -1"),
        ("batched", s.but(dims=None), {}, "null dims"), ("constrained", s.but(w=None), {}, "null parameter struct"),
        ("batched", s, dict(ws_bytes=1024), "workspace 1024 <"), ("batched", s.but(beamk=0), {}, "K=0"), ("sampled", s.but(temps=()), {}, "workspace"),
        # sampled
        ("sampled", s.but(smp=Smp(method=5, seed=1)), {}, "sampling method 5"), ("sampled", s.but(smp=Smp(method=2, sample_topk=0, seed=1)), {}, "sample_topk 0"),
        ("sampled", s.but(smp=Smp(method=2, sample_topk=V + 1, seed=1)), {}, "sample_topk 84"),
        ("sampled", s.but(smp=Smp(method=3, sample_topp=0.0, seed=1)), {}, "sample_topp 0"), ("sampled", s.but(smp=Smp(method=3, sample_topp=1.5, seed=1)), {}, "sample_topp 1.5"),
        ("sampled", s.but(smp=Smp(method=4, seed=1)), {}, "ancestral sampling is defined for beamk == 1"),
        ("constrained", s.but(beamk=1, smp=Smp(method=4, seed=1), con=Con(n_banned=1, banned=P)), {}, "ancestral sampling does not combine with constraints"),
        # constrained
        ("constrained", s.but(con=Con(topg=V + 1)), {}, "topg 84 outside"), ("constrained", s.but(con=Con(topg=-1)), {}, "topg -1 outside"),
        ("constrained", s.but(con=Con(topg=2), smp=Smp(method=1, seed=1)), {}, "topg 2 combines with"),
        ("constrained", s.but(con=Con(max_prefix=S + 1, prefix=P, prefix_len=P)), {}, "max_prefix 7 outside"),
        ("constrained", s.but(con=Con(max_prefix=2, prefix_len=P)), {}, "null pointer (prefix / prefix_len"),
        ("constrained", s.but(con=Con(n_banned=V + 1, banned=P)), {}, "n_banned 84 outside"), ("constrained", s.but(con=Con(n_banned=2)), {}, "banned with n_banned 2"),
        ("constrained", s.but(beamk=1025, con=Con(topg=2)), {}, "beamk 1025 above 1024"),
        # history
        ("history", s.but(hist=Hist(no_repeat_ngram=-1)), {}, "no_repeat_ngram -1"), ("history", s.but(hist=Hist(min_length=S + 1)), {}, "min_length 7 outside"),
        ("history", s.but(hist=Hist(repetition_penalty=-1.0)), {}, "repetition_penalty -1"),
        ("history", s.but(hist=Hist(repetition_penalty=float("inf"))), {}, "repetition_penalty inf"),
        ("history", s.but(S=128, hist=Hist(no_repeat_ngram=2)), {}, "max_gen_length 128 is over the limit"),
        ("history", s.but(beamk=1, smp=Smp(method=4, seed=1), hist=Hist(min_length=2)), {}, "ancestral sampling does not combine with the history rules"),
        # groups
        ("groups", s.but(grp=Grp(groups=-1)), {}, "groups -1 is negative"), ("groups", s.but(grp=Grp(groups=2, diversity_penalty=-0.5)), {}, "diversity_penalty -0.5"),
        ("groups", s.but(grp=Grp(groups=3, diversity_penalty=0.5)), {}, "beamk 4 is not a multiple of groups 3"),
        ("groups", s.but(grp=Grp(groups=2), smp=Smp(method=2, sample_topk=3, seed=1)), {}, "groups combine with \"beam\" sampling only"),
        ("groups", s.but(grp=Grp(groups=2), smp=Smp(method=0, decoder_noise=0.5, seed=1)), {}, "groups do not combine with decoder_noise"),
        ("groups", s.but(grp=Grp(groups=2), con=Con(topg=2)), {}, "groups do not combine with topg 2"),
        ("groups", s.but(grp=Grp(groups=2), con=Con(max_prefix=2, prefix=P, prefix_len=P)), {}, "groups do not combine with a forced prefix"),
        # required
        ("required", s.but(req=Req(max_required=9, words=P, n_words=P)), {}, "max_required 9 outside 0..8"), ("required", s.but(req=Req(max_required=-1)), {}, "max_required -1"),
        ("required", s.but(req=Req(max_required=2, n_words=P)), {}, "null pointer (words / n_words"), ("required", s.but(req=req2), dict(req_met=None), "null pointer (req_met"),
        ("required", s.but(beamk=257, req=req2), {}, "beamk 257 above 256"), ("required", s.but(S=2, req=Req(max_required=3, words=P, n_words=P)), {}, "max_required 3 above max_gen_length 2"),
        ("required", s.but(req=req2, smp=Smp(method=1, seed=1)), {}, "required words combine with \"beam\" sampling only"),
        ("required", s.but(req=req2, con=Con(topg=2)), {}, "required words do not combine with topg 2"),
    ]
    e = _ensemble()
    three = _ensemble()
    three.ens.members = 9
    other = _ensemble()
    other.ens.dims[1].contents.B = 3
    no_ann = _ensemble()
    no_ann.ens.ann[1] = None
    cases += [
        ("ensemble", three, {}, "members 9 outside"), ("ensemble", other, {}, "B=3"), ("ensemble", no_ann, {}, "null pointer for member 1"),
        ("ensemble", _ensemble(weights=(0.5, 0.4)), {}, "sum"), ("ensemble", _ensemble(weights=(1.5, -0.5)), {}, "weight[1]"), ("ensemble", _ensemble(combine=2), {}, "combine 2"),
        ("ensemble", e.but(con=Con(topg=2)), {}, "topg 2 does not combine with an ensemble"),
        ("ensemble", e.but(con=Con(max_prefix=2, prefix=P, prefix_len=P)), {}, "a forced prefix (max_prefix 2)"),
        ("ensemble", e.but(hist=Hist(repetition_penalty=1.2)), {}, "repetition_penalty 1.2 does not combine"), ("ensemble", e.but(hist=Hist(min_length=S + 1)), {}, "min_length 7"),
        ("ensemble", e.but(con=Con(n_banned=V + 1, banned=P)), {}, "n_banned 84"), ("ensemble", e.but(temps=(0.0,)), {}, "temperature 0"),
        ("ensemble", e, dict(outs=(None,) + (P,) * 7), "null pointer"), ("ensemble", e, dict(ws_bytes=4096), "workspace 4096 <"),
    ]
    return cases


def test_old_refusals_come_back_word_for_word():
    """every refusing call through its old entry and through sat_beam_search with the equivalent descriptor: the same status, and the same
    message after the leading name (the old entries say their own, the new one says beam_search)"""
    cases = _refusals()
    assert all(sum(1 for c in cases if c[0] == entry) >= 2 for entry in BC.ENTRIES)
    for entry, parts, kw, word in cases:
        (rc_old, msg_old), (rc_new, msg_new) = _both(entry, parts, **kw)
        assert rc_old != 0 and word in msg_old, (entry, word, rc_old, msg_old)
        assert rc_new == rc_old and _tail(msg_new) == _tail(msg_old), (entry, word, msg_old, msg_new)
        head = msg_old.split(": ", 1)[0]
        if head.startswith("beam_search_"):                  # a check made under the caller's name
            assert head == "beam_search_" + entry and msg_new.split(": ", 1)[0] == "beam_search"
        else:
            assert msg_new == msg_old


def test_refusals_only_a_descriptor_can_express():
    """a null descriptor or output struct, and an ensemble next to what does not combine with it: each message names its field"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    e, s = _ensemble(), _single()
    out = L.BeamSearchOut(*((P,) * 9))
    assert lib.sat_beam_search(None, C.byref(out), P, BIG, None) != 0 and "null descriptor" in lib.sat_last_error().decode()
    assert lib.sat_beam_search(C.byref(BC.descriptor(L, s)), None, P, BIG, None) != 0 and "null output struct" in lib.sat_last_error().decode()
    assert lib.sat_beam_search_desc_workspace_bytes(None) == 0 and "null descriptor" in lib.sat_last_error().decode()
    Smp = L.BeamSampling
    cases = [(e.but(dims=s.dims), "d / w / ann"), (e.but(w=s.w), "d / w / ann"), (e.but(ann=P), "d / w / ann"),
             (e.but(smp=Smp(method=1, seed=1)), "sampling method 1"), (e.but(smp=Smp(method=3, sample_topp=0.9, seed=1)), "sampling method 3"),
             (e.but(smp=Smp(method=0, decoder_noise=0.5, seed=1)), "decoder_noise 0.5"),
             (e.but(grp=L.BeamGroups(groups=2, diversity_penalty=0.5)), "groups 2"),
             (e.but(req=L.BeamRequired(max_required=2, words=P, n_words=P)), "max_required 2")]
    for parts, word in cases:
        rc = BC.new_call(L, parts, OUTS, P, P, BIG, None)
        msg = lib.sat_last_error().decode()
        assert rc != 0 and msg.startswith("beam_ensemble: ") and word in msg and "ensemble" in msg, (word, rc, msg)
        n, qmsg = _query(parts)
        assert n == 0 and qmsg == msg
    # what is off is no refusal: the plain method without noise, groups 0 / 1, max_required 0 (the search then stops at the small workspace)
    for parts in (e.but(smp=Smp(method=0, seed=1)), e.but(grp=L.BeamGroups(groups=1)), e.but(req=L.BeamRequired(max_required=0))):
        assert BC.new_call(L, parts, OUTS, P, P, 16, None) != 0 and "workspace 16 <" in lib.sat_last_error().decode()
        assert _query(parts)[0] == _query(e)[0] > 0


def test_the_query_is_the_figure_the_search_compares_against():
    """positive for every family; one byte less and the search refuses, naming the workspace; equal to the old query where that one is
    exact and never above it; what the search refuses the query refuses, in the search's words"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    s, e = _single(), _ensemble()
    Con, Hist, Grp, Req = L.BeamConstraints, L.BeamHistory, L.BeamGroups, L.BeamRequired
    d = C.byref(s.dims)
    rule = Hist(no_repeat_ngram=2)
    req2 = Req(max_required=2, words=P, n_words=P)
    families = [("plain", s, lib.sat_beam_search_workspace_bytes(d, K), True),
                ("topg 3", s.but(con=Con(topg=3)), lib.sat_beam_search_constrained_workspace_bytes(d, K, 3), True),
                ("one rule", s.but(hist=rule), lib.sat_beam_search_history_workspace_bytes(d, K, 0, S), True),
                ("topg 3 and a rule", s.but(con=Con(topg=3), hist=rule), lib.sat_beam_search_history_workspace_bytes(d, K, 3, S), True),
                ("groups 2", s.but(grp=Grp(groups=2, diversity_penalty=0.5)), lib.sat_beam_search_groups_workspace_bytes(d, K, 2, S), False),
                ("required 2", s.but(req=req2), lib.sat_beam_search_required_workspace_bytes(d, K, S, 2), False),
                ("groups 2 with a rule", s.but(grp=Grp(groups=2, diversity_penalty=0.5), hist=rule), lib.sat_beam_search_groups_workspace_bytes(d, K, 2, S), False),
                ("ensemble", e, lib.sat_beam_search_ensemble_workspace_bytes(C.byref(e.ens), K, S), False)]
    sizes = {}
    for name, parts, old, exact in families:
        n, msg = _query(parts)
        assert n > 0 and old > 0, (name, n, old, msg)
        assert n == old if exact else n <= old, (name, n, old)
        rc = BC.new_call(L, parts, OUTS, P, P, n - 1, None)
        msg = lib.sat_last_error().decode()
        assert rc != 0 and "workspace %d < %d" % (n - 1, n) in msg, (name, msg)
        sizes[name] = n
    # every feature that keeps something in the workspace shows in the figure; the tables of a rule are the required words' tables
    assert sizes["plain"] < sizes["topg 3"] < sizes["topg 3 and a rule"] and sizes["plain"] < sizes["one rule"] == sizes["required 2"]
    assert sizes["plain"] < sizes["groups 2"] < sizes["groups 2 with a rule"] and sizes["ensemble"] > sizes["one rule"]
    assert _query(s.but(hist=Hist(repetition_penalty=1.0)))[0] == sizes["plain"]            # every rule off: no tables
    for parts, word in ((s.but(req=Req(max_required=9, words=P, n_words=P)), "max_required 9"), (s.but(con=Con(topg=V + 1)), "topg 84"),
                        (s.but(beamk=0), "K=0"), (s.but(S=-1), "max_gen_length=-1"), (s.but(temps=(0.0,)), "temperature 0"), (s.but(ann=None), "null pointer"),
                        (s.but(grp=Grp(groups=3)), "not a multiple"), (e.but(hist=Hist(repetition_penalty=1.3)), "repetition_penalty"),
                        (s.but(beamk=1, smp=L.BeamSampling(method=4, seed=1), hist=rule), "ancestral")):
        n, msg = _query(parts)
        rc = BC.new_call(L, parts, OUTS, P, P, BIG, None)
        said = lib.sat_last_error().decode()
        assert n == 0 and word in msg and rc != 0 and word in said, (word, n, msg, said)
        if "workspace" not in msg:                           # (that message quotes the bytes the caller brought)
            assert _tail(said) == _tail(msg), (msg, said)
    # the query reads no output: required words without req_met are the search's refusal alone
    assert _query(s.but(req=req2))[0] > 0 and BC.new_call(L, s.but(req=req2), OUTS, None, P, BIG, None) != 0


# ---------------------------------------------------------------------------------------------------------------- SearchOptions
def _public_surface():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, model as M, visualize as Z
    return [M.SAT.caption, M.SAT.forward, M.SAT.val_batch, M.SAT.caption_tokens, M.SAT.val_batch_stats, M.SAT.visualize, M.SAT.caption_image,
            M.SATDecoder.beam_decode_batched, M.SATDecoder.beam_decode, M.SATDecoder._beam_search_device, E.caption_tokens, E.val_batch_stats, Z.visualize,
            Z.caption_image]


def test_search_options_name_every_option_once_with_the_public_defaults():
    from sat_amd import constraints as Cn
    fields = {f.name: f.default for f in dataclasses.fields(Cn.SearchOptions)}
    assert list(fields) == ["sample_method", "sample_topk", "sample_topp", "decoder_noise", "seed", "gumbel", "normals", "graph", "topg", "prefix", "banned",
                            "no_unk", "no_repeat_ngram", "min_length", "repetition_penalty", "beam_groups", "diversity_penalty", "required"]
    everywhere = set(fields) - {"seed", "gumbel", "normals", "graph"}          # the tables and the graph belong to the device half
    for fn in _public_surface():
        params = inspect.signature(fn).parameters
        assert everywhere <= set(params), (fn.__qualname__, everywhere - set(params))
        for name, default in fields.items():
            if name in params:
                assert params[name].default == default, (fn.__qualname__, name, params[name].default, default)
    opt = Cn.SearchOptions.from_kwargs(dict(self=1, beamk=3, topg=2, sample_method="topk", unrelated=5), seed=7)
    assert (opt.topg, opt.sample_method, opt.seed, opt.required) == (2, "topk", 7, None)
    with pytest.raises(dataclasses.FrozenInstanceError):
        opt.topg = 3
    assert set(opt.kwargs(Cn.check_ancestral)) == {"sample_method", "graph", "topg", "prefix", "banned", "no_unk", "no_repeat_ngram", "min_length",
                                                  "repetition_penalty"}


def test_resolve_raises_todays_value_errors():
    """one bad value per option: the text is the one the feature's own check raises; what is off resolves to four Nones"""
    from sat_amd import constraints as Cn
    stoi = {"<START>": 0, "<PAD>": 1, "<END>": 2, "<UNK>": 3}

    def resolve(beamk=K, S_=S, B=2, batched=True, **kw):
        return Cn.SearchOptions(**kw).resolve(stoi, V, B, beamk, S_, batched=batched)
    assert resolve() == (None, None, None, None)
    assert resolve(beam_groups=1, repetition_penalty=1.0, required=[[], []], no_repeat_ngram=0, batched=False) == (None, None, None, None)
    con, hist, grp, req = resolve(banned=[7], no_unk=True, min_length=2, beam_groups=2, diversity_penalty=0.25)
    assert (con.banned, hist.min_length, grp.groups, grp.diversity_penalty, req) == ([3, 7], 2, 2, 0.25, None)
    con, hist, grp, req = resolve(required=[[5, 6], []], no_repeat_ngram=2)
    assert (con, hist.no_repeat_ngram, grp, req.words) == (None, 2, None, [[5, 6], []])
    bad = [(dict(sample_method="nucleus", sample_topp=0), "sample_topp 0 outside (0, 1] (sample_method='nucleus')"),
           (dict(sample_method="ancestral"), "sample_method='ancestral' is defined for beamk=1 only (beamk=4): repeat the images to draw several samples"),
           (dict(sample_method="ancestral", beamk=1, graph=True), "sample_method='ancestral' is not replayed from a graph (graph=True)"),
           (dict(sample_method="ancestral", beamk=1, no_unk=True), "sample_method='ancestral' does not combine with topg / prefix / banned / no_unk"),
           (dict(topg=0), "topg=0 outside 1..V=83"), (dict(topg=2, sample_method="topk"), "topg combines with sample_method='beam' only, not 'topk'"),
           (dict(prefix=[2]), "<END> (id 2) in a prefix"), (dict(prefix=[[5], [6], [7]]), "3 prefixes for 2 images"),
           (dict(banned=[99]), "banned id 99 outside [0, V=83)"), (dict(banned=[2]), "<END> cannot be banned: no hypothesis could finish"),
           (dict(no_repeat_ngram=-1), "no_repeat_ngram=-1 is negative (0 = off)"), (dict(min_length=S + 1), "min_length=7 outside 0..max_gen_length=6"),
           (dict(repetition_penalty=0.0), "repetition_penalty=0.0 is not a positive finite number (1.0 = off)"),
           (dict(beam_groups=3), "beam_groups=3 does not divide beamk=4"), (dict(beam_groups=-1), "beam_groups=-1 is negative (None, 0 or 1 = off)"),
           (dict(beam_groups=2, diversity_penalty=-1.0), "diversity_penalty=-1.0 is not a finite number >= 0"),
           (dict(beam_groups=2, decoder_noise=0.5), "beam_groups does not combine with decoder_noise=0.5"),
           (dict(beam_groups=2, graph=True), "beam_groups is not replayed from a graph (graph=True)"),
           (dict(beam_groups=2, batched=False), "beam_groups=2 runs in the batched search only (beam_decode_batched), not in the per-image loop beam_decode"),
           (dict(required=[2]), "<END> (id 2) among the required words"), (dict(required=[5], sample_method="multinomial"),
                                                                          "required combines with sample_method='beam' only, not 'multinomial'"),
           (dict(required=[5], batched=False),
            "required words run in the batched search only (beam_decode_batched, max_gen_length >= 1), not in the per-image loop beam_decode")]
    for kw, text in bad:
        with pytest.raises(ValueError) as err:
            resolve(**kw)
        assert str(err.value) == text, kw
    # the order is the device half's: sample_topp, ancestral, constraints and history, groups, required words
    with pytest.raises(ValueError, match="topg=0"):
        resolve(topg=0, beam_groups=3, required=[2])
    with pytest.raises(ValueError, match="does not divide"):
        resolve(beam_groups=3, required=[2])


def test_the_picture_callers_refuse_before_any_picture_is_read():
    """visualize / caption_image run the whole sequence, "ancestral" and sample_topp included, in front of the loader"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, model as M, visualize as Z
    from oracle import sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over)))
    missing = ["/nonexistent.jpg"]
    for call in (lambda **kw: Z.caption_image(model, missing, **kw), lambda **kw: Z.visualize(model, missing, **kw), lambda **kw: model.caption_image(missing, **kw),
                 lambda **kw: model.visualize(missing, **kw)):
        with pytest.raises(ValueError, match="ancestral"):
            call(sample_method="ancestral", beamk=2)
        with pytest.raises(ValueError, match="sample_topp"):
            call(sample_method="nucleus", sample_topp=0, beamk=2)
        with pytest.raises(ValueError, match="beam_groups"):
            call(beam_groups=3, beamk=4)
    with pytest.raises(L.SatHipError, match="GPU only"):       # a call that resolves does reach the loader (its first check: a model on the CPU)
        Z.caption_image(model, missing, beamk=2)
