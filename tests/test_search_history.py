"""CPU: the history rules of the caption search ("History rules": no-repeat n-gram, minimum length, repetition penalty).
The CPU reference (tests/history_ref.py) against brute force and against the oracle's search, every ValueError of the Python surface,
and the C entry points refusing bad arguments before anything is launched."""
import ctypes as C
import os
import random
import re

import pytest
import torch

import history_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K, S = 83, 4, 9
TEMPS = [1.0, 0.7]


def test_blocked_words_against_a_brute_force_ngram_set():
    """1. a word is blocked exactly when history + [word] ends in an n-gram the history already holds"""
    rnd = random.Random(11)
    hits = 0
    for n in (1, 2, 3, 4):
        for length in range(0, 13):
            for _ in range(40):
                hist = [rnd.randrange(5) for _ in range(length)]
                have = {tuple(hist[p:p + n]) for p in range(length - n + 1)}
                want = {w for w in range(5) if length >= n - 1 and tuple((hist + [w])[-n:]) in have}
                assert HR.blocked_words(hist, n) == want, (hist, n)
                hits += len(want)
    assert hits > 1000
    assert HR.blocked_words([3, 1, 3], 0) == set()
    assert not HR.repeats_ngram([4, 5, 4, 6], 2) and HR.repeats_ngram([4, 5, 6, 4, 5], 2)
    assert not HR.repeats_ngram([4, 4, 4, 5], 1, free_from=3) and HR.repeats_ngram([4, 4, 4, 5, 4], 1, free_from=3)


def _decoder(layers=1, seed=None, **over):
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    hp = O.default_hparams(vocab_size=V, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40, decoder_layers=layers, **over)
    torch.manual_seed(3 + layers if seed is None else seed)
    return M.SATDecoder(hp).eval(), hp


@pytest.mark.parametrize("layers", [1, 2])
def test_reference_with_every_rule_off_is_the_oracle_search(layers):
    """2. captions, scores and perplexities identical on the shapes of test_gpu_constrained_search._setup"""
    from oracle import prng, sat_oracle as O
    dec, hp = _decoder(layers)
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    ann = torch.from_numpy(prng.uniform((9, 12, 32), 55, 0.0, 1.0)).reshape(9, 3, 4, 32).permute(0, 3, 1, 2).contiguous()
    kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True)
    with torch.no_grad():
        want = O.beam_search(sd, hp, ann, **kw)
        margins = {}
        got = HR.beam_search(sd, hp, ann, margins=margins, **kw)
    assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3]
    assert all(torch.equal(a, b) for x, y in zip(got[2], want[2]) for a, b in zip(x, y))
    assert len(margins["final"]) == 9 and len(margins["boundary"]) >= 9 * 2
    with torch.no_grad():                                  # and the rules do bite on this model
        ruled = HR.beam_search(sd, hp, ann, no_repeat_ngram=2, min_length=4, repetition_penalty=1.3, **kw)
    assert ruled[0] != want[0]
    assert not any(HR.repeats_ngram(c, 2) for caps in ruled[0] for c in caps) and min(len(c) for caps in ruled[0] for c in caps) >= 4


def test_resolve_history_raises_every_value_error():
    """3. and the "off" spellings return None"""
    from sat_amd import constraints as Cn
    r = Cn.resolve_history
    for kw in (dict(), dict(no_repeat_ngram=None, min_length=None, repetition_penalty=None), dict(no_repeat_ngram=0), dict(min_length=0),
               dict(repetition_penalty=1.0), dict(no_repeat_ngram=0, min_length=0, repetition_penalty=1.0)):
        assert r(V, K, S, "beam", None, 0, **kw) is None
    assert r(V, K, 500, "beam", None, 0) is None                             # a long search without a rule is nobody's business here
    got = r(V, K, S, "nucleus", None, 2, no_repeat_ngram=3, min_length=S, repetition_penalty=1.3)
    assert (got.no_repeat_ngram, got.min_length) == (3, S) and abs(got.repetition_penalty - 1.3) < 1e-12
    st = got.device_struct()
    assert (st.no_repeat_ngram, st.min_length, st.reserved) == (3, S, 0) and abs(st.repetition_penalty - 1.3) < 1e-6
    bad = [dict(no_repeat_ngram=-1), dict(min_length=-1), dict(min_length=S + 1), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.2),
           dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            r(V, K, S, "beam", None, 0, **kw)
    with pytest.raises(ValueError, match="128"):                             # max_gen_length + 1 > SAT_CAPTION_MAX_LEN
        r(400, K, 128, "beam", None, 0, no_repeat_ngram=2)
    assert r(400, K, 127, "beam", None, 0, no_repeat_ngram=2) is not None
    # enough words must stay selectable: V - 4 specials - banned - max_gen_length >= max(beamk, topg or 1)
    assert r(V, K, S, "beam", None, V - 4 - S - K, no_repeat_ngram=2) is not None
    with pytest.raises(ValueError, match="unmasked"):
        r(V, K, S, "beam", None, V - 4 - S - K + 1, no_repeat_ngram=2)
    assert r(V, K, S, "beam", 7, V - 4 - S - 7, min_length=2) is not None
    with pytest.raises(ValueError, match="unmasked"):
        r(V, K, S, "beam", 7, V - 4 - S - 6, min_length=2)
    with pytest.raises(ValueError, match="ancestral"):
        r(V, 1, S, "ancestral", None, 0, min_length=2)
    # resolve and check_ancestral keep today's behaviour for today's arguments
    _, hp = _decoder()
    assert Cn.resolve(hp.vocab_stoi, V, 3, K, S) is None
    assert Cn.resolve_all(hp.vocab_stoi, V, 3, K, S) == (None, None)
    con, hist = Cn.resolve_all(hp.vocab_stoi, V, 3, K, S, no_unk=True, banned=[5], no_repeat_ngram=2)
    assert con.banned == sorted([5, int(hp.vocab_stoi["<UNK>"])]) and hist.no_repeat_ngram == 2
    with pytest.raises(ValueError, match="unmasked"):                        # <UNK> is a special: only the other banned ids count
        Cn.resolve_all(hp.vocab_stoi, V, 3, K, S, no_unk=True, banned=list(range(1, 1 + V - 4 - S - K + 1)), no_repeat_ngram=2)
    Cn.resolve_all(hp.vocab_stoi, V, 3, K, S, no_unk=True, banned=list(range(1, 1 + V - 4 - S - K)), no_repeat_ngram=2)
    Cn.check_ancestral("ancestral", 1)
    Cn.check_ancestral("beam", 4, False, None, None, None, False, 2, 3, 1.3)


def test_python_surface_raises_before_touching_a_gpu():
    """3./4. CPU tensors: a call that got past the checks would fail with SatHipError (no CPU fallback); ancestral refuses every rule"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, evaluation as E, model as M, visualize as Z
    from oracle import sat_oracle as O
    import numpy as np
    dec, hp = _decoder()
    ann = torch.zeros(3, 12, 32)
    bad = [dict(no_repeat_ngram=-2), dict(min_length=S + 1), dict(min_length=-1), dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")),
           dict(no_repeat_ngram=2, banned=list(range(1, 1 + V - 4 - S - K + 1)))]
    for kw in bad:
        for fn in (dec.beam_decode, dec.beam_decode_batched):
            with pytest.raises(ValueError):
                fn(ann, (3, 4), beamk=K, max_gen_length=S, **kw)
    for kw in (dict(no_repeat_ngram=2), dict(min_length=3), dict(repetition_penalty=1.2), dict(no_repeat_ngram=0), dict(repetition_penalty=1.0)):
        with pytest.raises(ValueError, match="ancestral"):                   # 4. any of the three keywords, an "off" value included
            dec.beam_decode_batched(ann, (3, 4), beamk=1, max_gen_length=S, sample_method="ancestral", **kw)
    with pytest.raises(ValueError, match="128"):
        dec.beam_decode_batched(ann, (3, 4), beamk=1, max_gen_length=128, no_repeat_ngram=2)
    with pytest.raises(L.SatHipError):                                       # well-formed rules reach the GPU check
        dec.beam_decode_batched(ann, (3, 4), beamk=K, max_gen_length=S, no_repeat_ngram=2, min_length=3, repetition_penalty=1.3)
    with pytest.raises(L.SatHipError):
        dec.beam_decode_batched(ann, (3, 4), beamk=K, max_gen_length=S, no_repeat_ngram=0, min_length=0, repetition_penalty=1.0)
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over)))
    img = torch.zeros(2, 3, 64, 64)
    caps, lens = torch.zeros(2, 3, 9, dtype=torch.int64), torch.full((2, 3), 4)
    pic = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(ValueError):
        model.caption(img, no_repeat_ngram=-1)
    with pytest.raises(ValueError):
        model.caption(img, beamk=1, sample_method="ancestral", min_length=2)
    with pytest.raises(ValueError):
        model.val_batch((img, caps, lens), min_length=33)
    with pytest.raises(ValueError):
        E.caption_tokens(model, img, repetition_penalty=-1.0)
    with pytest.raises(ValueError):
        model.val_batch_stats((img, caps, lens), max_gen_length=130, no_repeat_ngram=3)
    with pytest.raises(ValueError):
        E.evaluate(model, [(img, caps, lens)], min_length=40)
    with pytest.raises(ValueError):
        Z.caption_image(model, pic, repetition_penalty=0.0)
    with pytest.raises(ValueError):
        model.visualize(pic, no_repeat_ngram=2, max_gen_length=32, banned=list(range(1, 1 + 60 - 4 - 32 - 3 + 1)))


def test_header_and_library_declare_the_history_entry_points():
    """5. three new symbols, the version stays 23"""
    from sat_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    assert "#define SAT_HIP_ABI_VERSION 23" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sat_beam_search_history_workspace_bytes", "sat_beam_search_history", "sat_beam_history_scores"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.SYMBOLS
    assert re.search(r"typedef struct sat_beam_history \{[^}]*no_repeat_ngram;[^}]*min_length;[^}]*repetition_penalty;[^}]*reserved;[^}]*\} sat_beam_history;", code)
    assert C.sizeof(L.BeamHistory) == 16
    assert L.lib().sat_abi_version() == 23


def _call_search(dec, hp, hist, con=None, method=0, mgl=S, B=2, beamk=K):
    """sat_beam_search_history on host pointers: every check under test runs before the first launch, nothing is dereferenced"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    dims = Dk.decoder_dims(B, beamk, 2, 12, 32, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    w, keep = dec._params_struct()
    ws_bytes = lib.sat_beam_search_history_workspace_bytes(C.byref(dims), beamk, 0, min(max(mgl, 0), 127))
    buf = torch.zeros(64, dtype=torch.int32)
    p = buf.data_ptr()
    temps = (C.c_float * 1)(1.0)
    ids = (C.c_int32 * 4)(*[int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    smp = L.BeamSampling(method=method, sample_topk=3, seed=1) if method else None
    rc = lib.sat_beam_search_history(C.byref(dims), C.byref(w), p, beamk, mgl, temps, 1, ids, C.byref(smp) if smp is not None else None,
                                     C.byref(con) if con is not None else None, C.byref(hist) if hist is not None else None, p, p, p, p, p, p, p, p, p,
                                     ws_bytes, None)
    return rc, lib.sat_last_error().decode()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """6. SAT_EINVAL with a message; the pointers are never followed"""
    from sat_amd import _lib as L, decoder as Dk
    dec, hp = _decoder()
    H = L.BeamHistory
    cases = [(H(no_repeat_ngram=-1), S, "no_repeat_ngram"), (H(min_length=-1), S, "min_length"), (H(min_length=S + 1), S, "min_length"),
             (H(repetition_penalty=-1.0), S, "repetition_penalty"), (H(repetition_penalty=float("inf")), S, "repetition_penalty"),
             (H(repetition_penalty=float("nan")), S, "repetition_penalty"), (H(repetition_penalty=-0.0), S, "repetition_penalty"),
             (H(no_repeat_ngram=2), 128, "max_gen_length"), (H(min_length=1, repetition_penalty=1.0), 200, "max_gen_length")]
    for hist, mgl, word in cases:
        rc, msg = _call_search(dec, hp, hist, mgl=mgl)
        assert rc != 0 and "beam_history" in msg and word in msg, (word, rc, msg)
    rc, msg = _call_search(dec, hp, H(no_repeat_ngram=2), method=4, beamk=1)
    assert rc != 0 and "ancestral" in msg
    rc, msg = _call_search(dec, hp, H(no_repeat_ngram=2), con=L.BeamConstraints(topg=-1))     # the constraints' own checks still run
    assert rc != 0 and "topg" in msg
    # the workspace query: the constrained figure plus two (B * beamk, max_gen_length + 1) int32 tables
    lib = L.lib()
    dims = Dk.decoder_dims(2, K, 2, 12, 32, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    base = lib.sat_beam_search_constrained_workspace_bytes(C.byref(dims), K, 3)
    assert lib.sat_beam_search_history_workspace_bytes(C.byref(dims), K, 3, S) >= base + 2 * 2 * K * (S + 1) * 4
    assert lib.sat_beam_search_history_workspace_bytes(C.byref(dims), K, 3, 128) == 0 and "max_gen_length" in lib.sat_last_error().decode()
    assert lib.sat_beam_search_history_workspace_bytes(C.byref(dims), K, V + 1, S) == 0 and "topg" in lib.sat_last_error().decode()

    # sat_beam_history_scores
    p = torch.zeros(64, dtype=torch.int32).data_ptr()

    def scores(rules, rows=2, v=V, T=1.0, stride=8, logits=p, hist=p, hist_len=p, out=p, n_masked=2, masked=p):
        rc = lib.sat_beam_history_scores(logits, rows, v, T, masked, n_masked, None, hist, hist_len, stride, C.byref(rules) if rules is not None else None, 3,
                                         2, out, None)
        return rc, lib.sat_last_error().decode()
    ok = H(no_repeat_ngram=2, min_length=1, repetition_penalty=1.3)
    bad = [(dict(rules=H(no_repeat_ngram=-3)), "no_repeat_ngram"), (dict(rules=H(min_length=-1)), "min_length"),
           (dict(rules=H(repetition_penalty=-2.0)), "repetition_penalty"), (dict(rules=H(repetition_penalty=float("nan"))), "repetition_penalty"),
           (dict(rules=ok, stride=129), "hist_stride"), (dict(rules=ok, stride=-1), "hist_stride"), (dict(rules=ok, rows=0), "size"),
           (dict(rules=ok, v=0), "size"), (dict(rules=ok, T=0.0), "temperature"), (dict(rules=None), "null pointer"),
           (dict(rules=ok, logits=None), "null pointer"), (dict(rules=ok, hist=None), "null pointer"), (dict(rules=ok, hist_len=None), "null pointer"),
           (dict(rules=ok, out=None), "null pointer"), (dict(rules=ok, masked=None), "null pointer")]
    for kw, word in bad:
        rc, msg = scores(**kw)
        assert rc != 0 and "beam_history_scores" in msg and word in msg, (word, rc, msg)
