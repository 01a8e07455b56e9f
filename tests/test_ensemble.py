"""CPU: ensemble decoding ("Ensemble decoding").  The reference tests/ensemble_ref.py on hand-computed cases and against
tests/history_ref.py where the two must agree, every ``ValueError`` of ``sat_amd.ensemble.Ensemble`` and every refusal of the C entry
points before anything is launched.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import ensemble_ref as ER
import history_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K, S = 83, 4, 9
TEMPS = [1.0, 0.7]
#: the three members of the heterogeneous ensemble (test_gpu_ensemble.py, test 4): hyper-parameter overrides and the (h, w) of the map
HETERO = [(dict(encoder_dim=32, decoder_dim=40, decoder_layers=1), (3, 4)),
          (dict(encoder_dim=48, decoder_dim=40, decoder_layers=2), (2, 3)),
          (dict(encoder_dim=32, decoder_dim=56, decoder_layers=1, deep_output=True), (3, 4))]


def build_member(seed, over, hw, ann_seed=55):
    """(decoder on the CPU, hparams, annotations (9, L, D)): built after ``torch.manual_seed(seed)``"""
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import prng, sat_oracle as O
    hp = O.default_hparams(**dict(dict(vocab_size=V, embed_dim=24, attention_dim=16), **over))
    torch.manual_seed(seed)
    dec = M.SATDecoder(hp).eval()
    ann = torch.from_numpy(prng.uniform((9, hw[0] * hw[1], hp.encoder_dim), ann_seed, 0.0, 1.0))
    return dec, hp, ann


def hetero_members(seed, specs=HETERO):
    """member i of the heterogeneous ensemble is built after ``torch.manual_seed(seed + 1000 i)`` on annotations of its own (seed 55 + i)"""
    return [build_member(seed + 1000 * i, over, hw, 55 + i) + (hw,) for i, (over, hw) in enumerate(specs)]


def reference_member(dec, hp, ann, hw):
    """what ``ensemble_ref.beam_search`` takes: (state dict, hparams, annotations as the image (B, D, h, w))"""
    sd = {k: v.detach().cpu().clone() for k, v in dec.state_dict().items()}
    return sd, hp, ann.cpu().reshape(ann.shape[0], hw[0], hw[1], ann.shape[2]).permute(0, 3, 1, 2).contiguous()


def test_combine_on_hand_computed_cases():
    """1. V = 4, M = 2: member 0 is (.1, .2, .3, .4), member 1 the same reversed"""
    z0 = torch.log(torch.tensor([[1.0, 2.0, 3.0, 4.0]])); z1 = torch.log(torch.tensor([[4.0, 3.0, 2.0, 1.0]]))
    lg = lambda xs: torch.tensor([[math.log(x) for x in xs]], dtype=torch.float64)
    got = ER.combine([z0, z1], [0.5, 0.5], "arithmetic", 1.0)
    assert got.dtype == torch.float64 and torch.allclose(got, lg([0.25] * 4), atol=1e-7)
    assert torch.allclose(ER.combine([z0, z1], [0.75, 0.25], "arithmetic", 1.0), lg([0.175, 0.225, 0.275, 0.325]), atol=1e-7)
    assert torch.allclose(ER.combine([z0, z1], [0.5, 0.5], "geometric", 1.0), lg([0.2, math.sqrt(0.06), math.sqrt(0.06), 0.2]), atol=1e-7)
    assert torch.allclose(ER.combine([z0, z1], [0.75, 0.25], "geometric", 1.0),
                          lg([0.1 ** 0.75 * 0.4 ** 0.25, 0.2 ** 0.75 * 0.3 ** 0.25, 0.3 ** 0.75 * 0.2 ** 0.25, 0.4 ** 0.75 * 0.1 ** 0.25]), atol=1e-7)
    # T = 0.5 squares the probabilities before they are normalised: (1, 4, 9, 16) / 30
    assert torch.allclose(ER.combine([z0, z1], [0.5, 0.5], "arithmetic", 0.5), lg([17 / 60, 13 / 60, 13 / 60, 17 / 60]), atol=1e-7)
    for mode in ("arithmetic", "geometric"):
        # a zero weight: the other member alone, whatever the skipped member holds (NaN included); M = 1 is log_softmax
        junk = torch.full((1, 4), float("nan"))
        want = torch.log_softmax(z0.double() / 0.7, dim=1)
        assert torch.allclose(ER.combine([z0, junk], [1.0, 0.0], mode, 0.7), want, atol=1e-12)
        assert torch.allclose(ER.combine([junk, z0], [0.0, 1.0], mode, 0.7), want, atol=1e-12)
        assert torch.allclose(ER.combine([z0], [1.0], mode, 0.7), want, atol=1e-12)
    # a member that is arbitrarily sure of word 0 (logits +-60): the mixture stays finite, and is bounded below by the other member's share
    peaked = torch.tensor([[60.0, -60.0, -60.0, -60.0]])
    got = ER.combine([peaked, z1], [0.5, 0.5], "arithmetic", 0.7)
    floor = torch.log_softmax(z1.double() / 0.7, dim=1) + math.log(0.5)
    assert torch.isfinite(got).all() and (got >= floor - 1e-12).all() and float(got[0, 1] - floor[0, 1]) < 1e-12
    assert abs(float(got[0, 0]) - math.log(0.5 + 0.5 * float(torch.softmax(z1.double() / 0.7, 1)[0, 0]))) < 1e-12
    geo = ER.combine([peaked, z1], [0.5, 0.5], "geometric", 0.7)
    assert torch.isfinite(geo).all() and float(geo[0, 1]) < -80.0


def _identical_captions(a, b, tol):
    assert a[0] == b[0]
    for i in (1, 3):
        for x, y in zip(a[i], b[i]):
            for u, v in zip(x, y):
                assert abs(u - v) <= tol * max(1.0, abs(u)), (i, u, v)
    assert all(torch.allclose(u, v, atol=tol) for x, y in zip(a[2], b[2]) for u, v in zip(x, y))


@pytest.mark.parametrize("layers", [1, 2])
def test_reference_with_one_distinct_member_is_the_history_reference(layers):
    """2. one member, or the same member twice at (0.5, 0.5), in both modes: captions and list order equal history_ref.beam_search,
    scores within 1e-5; without and with the rules an ensemble takes"""
    dec, hp, ann = build_member(3 + layers, dict(encoder_dim=32, decoder_dim=40, decoder_layers=layers), (3, 4))
    mem = reference_member(dec, hp, ann, (3, 4))
    for rules in (dict(), dict(no_repeat_ngram=2, min_length=3)):
        kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, rescore_method="LN", return_all=True, **rules)
        with torch.no_grad():
            want = HR.beam_search(*mem, **kw)
            for mode in ("arithmetic", "geometric"):
                _identical_captions(ER.beam_search([mem], [1.0], mode, **kw), want, 1e-5)
                _identical_captions(ER.beam_search([mem, mem], [0.5, 0.5], mode, **kw), want, 1e-5)


def test_reference_bans_words():
    dec, hp, ann = build_member(4, dict(encoder_dim=32, decoder_dim=40, decoder_layers=1), (3, 4))
    mem = reference_member(dec, hp, ann, (3, 4))
    kw = dict(beamk=K, max_gen_length=S, temperature=TEMPS, return_all=True)
    with torch.no_grad():
        plain = ER.beam_search([mem], [1.0], "arithmetic", **kw)
        word = plain[0][0][0][0]
        got = ER.beam_search([mem], [1.0], "arithmetic", banned=[word], **kw)
    assert any(word in c for caps in plain[0] for c in caps) and not any(word in c for caps in got[0] for c in caps)


def test_ensemble_raises_every_value_error_without_a_gpu():
    """3. construction and every refused keyword, before anything is launched (CPU tensors: a call that got past the checks would fail
    with SatHipError, there is no CPU fallback)"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, evaluation as E, model as M
    from sat_amd.ensemble import Ensemble
    from oracle import sat_oracle as O
    a, hp, ann = build_member(3, dict(encoder_dim=32, decoder_dim=40), (3, 4))
    b, _, _ = build_member(4, dict(encoder_dim=32, decoder_dim=56, deep_output=True), (3, 4))
    other = build_member(5, dict(encoder_dim=32, decoder_dim=40, vocab_size=V + 1), (3, 4))[0]
    renamed = build_member(5, dict(encoder_dim=32, decoder_dim=40), (3, 4))[0]
    renamed.hp.vocab_stoi = dict(renamed.hp.vocab_stoi, **{"zebra": 5})
    bad = [(dict(models=[]), "members"), (dict(models=[a] * 9), "members"), (dict(models=[a, other]), "vocabulary"), (dict(models=[a, renamed]), "vocabulary"),
           (dict(models=[a, b], weights=[1.0]), "weights"), (dict(models=[a, b], weights=[0.5, 0.25, 0.25]), "weights"),
           (dict(models=[a, b], weights=[1.5, -0.5]), "weight"), (dict(models=[a, b], weights=[0.0, 0.0]), "every weight is 0"),
           (dict(models=[a, b], weights=[float("nan"), 1.0]), "weight"), (dict(models=[a, b], combine="harmonic"), "combine")]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            Ensemble(**kw)
    ens = Ensemble([a, b], weights=[3, 1], combine="geometric")
    assert ens.weights == [0.75, 0.25] and Ensemble([a, b, a]).weights == [1 / 3] * 3 and Ensemble([a]).weights == [1.0]
    assert ens.hp is a.hp and ens.pad_idx == a.pad_idx and ens.embedding is a.embedding and ens.eval() is ens
    anns = [ann, ann]
    refused = [(dict(sample_method="multinomial"), "sample_method"), (dict(sample_method="nucleus"), "sample_method"), (dict(sample_method="ancestral", beamk=1), "sample_method"),
               (dict(topg=2), "topg"), (dict(prefix=[5, 6]), "prefix"), (dict(repetition_penalty=1.2), "repetition_penalty"), (dict(beam_groups=2), "beam_groups"),
               (dict(decoder_noise=0.2), "decoder_noise"), (dict(graph=True), "graph")]
    for e in (ens, Ensemble([a])):                  # one member delegates, after the same refusals
        for kw, word in refused:
            with pytest.raises(ValueError, match=word):
                e.beam_decode_batched(anns[:len(e.models)], (3, 4), **dict(dict(beamk=K, max_gen_length=S), **kw))
            dev = dict(dict(beamk=K, max_gen_length=S, temperature=1.0, sample_method="beam", sample_topk=3, decoder_noise=None, seed=None, gumbel=None,
                            normals=None, graph=False), **kw)
            with pytest.raises(ValueError, match=word):
                e._beam_search_device(anns[:len(e.models)], **dev)
    with pytest.raises(ValueError, match="beam_decode"):
        ens.beam_decode_batched(anns, (3, 4), beamk=K, max_gen_length=0)
    with pytest.raises(ValueError, match="min_length"):
        ens.beam_decode_batched(anns, (3, 4), beamk=K, max_gen_length=S, min_length=S + 1)
    with pytest.raises(ValueError, match="END"):
        ens.beam_decode_batched(anns, (3, 4), beamk=K, max_gen_length=S, banned=[int(hp.vocab_stoi["<END>"])])
    with pytest.raises(ValueError, match="mbr_corpus"):
        ens.beam_decode_batched(anns, (3, 4), beamk=K, max_gen_length=S, rescore_method="MBR")
    for kw in (dict(), dict(no_repeat_ngram=2, min_length=3, no_unk=True, banned=[7]), dict(repetition_penalty=1.0, beam_groups=1, decoder_noise=0.0)):
        with pytest.raises(L.SatHipError):          # what an ensemble takes reaches the GPU check
            ens.beam_decode_batched(anns, (3, 4), beamk=K, max_gen_length=S, temperature=TEMPS, **kw)
    # the evaluation surface, with whole models
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(5)
    m0 = M.SAT(**vars(O.default_hparams(**over)))
    m1 = M.SAT(**vars(O.default_hparams(**dict(over, decoder_layers=2))))
    full = Ensemble([m0, m1])
    img = torch.zeros(2, 3, 64, 64)
    caps, lens = torch.zeros(2, 3, 9, dtype=torch.int64), torch.full((2, 3), 4)
    with pytest.raises(ValueError, match="sample_method"):
        full.caption(img, beamk=3, sample_method="topk")
    with pytest.raises(ValueError, match="beam_decode"):
        full.caption(img, beamk=3, max_gen_length=0)
    with pytest.raises(ValueError, match="topg"):
        full.val_batch((img, caps, lens), beamk=3, topg=2)
    with pytest.raises(ValueError, match="graph"):
        full.caption_tokens(img, beamk=3, graph=True)
    with pytest.raises(ValueError, match="prefix"):
        full.val_batch_stats((img, caps, lens), beamk=3, prefix="a photo")
    with pytest.raises(ValueError, match="decoder_noise"):
        E.evaluate(full, [(img, caps, lens)], beamk=3, decoder_noise=0.1)
    with pytest.raises(ValueError, match="beam_groups"):
        E.evaluate(full, [(img, caps, lens)], beamk=4, beam_groups=2)
    pic = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(ValueError, match="topg"):
        full.visualize(pic, beamk=3, topg=2)
    with pytest.raises(ValueError, match="sample_method"):
        full.caption_image(pic, beamk=3, sample_method="nucleus")


def test_header_and_library_declare_the_ensemble_entry_points():
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    assert "#define SAT_HIP_ABI_VERSION 23" in text and "#define SAT_ENSEMBLE_MAX 8" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sat_beam_search_ensemble_workspace_bytes", "sat_beam_search_ensemble", "sat_beam_ensemble_scores"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.SYMBOLS
    assert re.search(r"typedef struct sat_beam_ensemble \{[^}]*\} sat_beam_ensemble;", code)
    assert L.ENSEMBLE_MAX == 8 and C.sizeof(L.BeamEnsemble) == 8 + 3 * 8 * 8 + 4 * 8
    assert L.lib().sat_abi_version() == 23


def _ensemble_struct(members, weights, combine=0, ann=None):
    """(sat_beam_ensemble over ``members`` = [(decoder, hparams, (L, D))], what it points into)"""
    from sat_amd import _lib as L, decoder as Dk
    p = torch.zeros(64, dtype=torch.int32)
    ens = L.BeamEnsemble(members=len(members), combine=combine)
    keep = [p]
    for i, (dec, hp, (Lc, D)) in enumerate(members[:L.ENSEMBLE_MAX]):
        dims = Dk.decoder_dims(2, K, 2, Lc, D, 16, 24, int(hp.decoder_dim), int(hp.vocab_size), 0, hp.deep_output, dec.pad_idx, 0, layers=int(hp.decoder_layers))
        w, tens = dec._params_struct()
        keep += [dims, w, tens]
        ens.dims[i], ens.params[i], ens.ann[i] = C.pointer(dims), C.pointer(w), p.data_ptr() if ann is None else ann
    for i, wt in enumerate(weights[:L.ENSEMBLE_MAX]):
        ens.weight[i] = wt
    return ens, keep


def _call_search(ens, con=None, hist=None, beamk=K):
    """sat_beam_search_ensemble on host pointers: every check under test runs before the first launch, nothing is dereferenced"""
    from sat_amd import _lib as L
    lib = L.lib()
    p = torch.zeros(64, dtype=torch.int32).data_ptr()
    temps = (C.c_float * 1)(1.0)
    ids = (C.c_int32 * 4)(1, 0, 2, 3)
    rc = lib.sat_beam_search_ensemble(C.byref(ens) if ens is not None else None, beamk, S, temps, 1, ids, C.byref(con) if con is not None else None,
                                      C.byref(hist) if hist is not None else None, p, p, p, p, p, p, p, p, p, 1 << 40, None)
    return rc, lib.sat_last_error().decode()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """4. an error status with a message naming the field; the device pointers are never followed"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    a, hpa, _ = build_member(3, dict(encoder_dim=32, decoder_dim=40), (3, 4))
    b, hpb, _ = build_member(4, dict(encoder_dim=48, decoder_dim=56, decoder_layers=2, deep_output=True), (2, 3))
    o, hpo, _ = build_member(5, dict(encoder_dim=32, decoder_dim=40, vocab_size=V + 1), (3, 4))
    ma, mb, mo = (a, hpa, (12, 32)), (b, hpb, (6, 48)), (o, hpo, (12, 32))
    p = torch.zeros(64, dtype=torch.int32).data_ptr()

    def struct(members=(ma, mb), weights=(0.5, 0.5), combine=0, edit=None, **kw):
        ens, keep = _ensemble_struct(list(members), list(weights), combine, **kw)
        if edit:
            edit(ens)
        return ens, keep

    def set_members(n):
        return lambda e: setattr(e, "members", n)

    def other_batch(e):
        e.dims[1].contents.B = 3

    cases = [(dict(edit=set_members(0)), "members"), (dict(edit=set_members(9)), "members"), (dict(edit=set_members(-1)), "members"),
             (dict(edit=lambda e: e.dims.__setitem__(1, C.POINTER(L.DecoderDims)())), "null pointer for member 1"),
             (dict(edit=lambda e: e.params.__setitem__(0, C.POINTER(L.DecoderParams)())), "null pointer for member 0"),
             (dict(edit=lambda e: e.ann.__setitem__(1, None)), "null pointer for member 1"),
             (dict(members=(ma, mo)), "V="), (dict(edit=other_batch), "B="),
             (dict(weights=(1.5, -0.5)), "weight[1]"), (dict(weights=(float("nan"), 1.0)), "weight[0]"), (dict(weights=(float("inf"), 0.0)), "weight[0]"),
             (dict(weights=(0.5, 0.4)), "sum"), (dict(weights=(0.5, 0.5001)), "sum"), (dict(weights=(0.0, 0.0)), "sum"),
             (dict(combine=2), "combine"), (dict(combine=-1), "combine")]
    for kw, word in cases:
        ens, keep = struct(**kw)
        rc, msg = _call_search(ens)
        assert rc != 0 and "beam_" in msg and word in msg, (word, rc, msg)
        assert lib.sat_beam_search_ensemble_workspace_bytes(C.byref(ens), K, S) == 0 and word in lib.sat_last_error().decode()
    rc, msg = _call_search(None)
    assert rc != 0 and "null ensemble" in msg
    ens, keep = struct()
    more = [(dict(con=L.BeamConstraints(topg=2)), "topg"), (dict(con=L.BeamConstraints(max_prefix=2, prefix=p, prefix_len=p)), "prefix"),
            (dict(hist=L.BeamHistory(repetition_penalty=1.2)), "repetition_penalty"), (dict(hist=L.BeamHistory(no_repeat_ngram=-1)), "no_repeat_ngram"),
            (dict(hist=L.BeamHistory(min_length=S + 1)), "min_length"), (dict(con=L.BeamConstraints(n_banned=V + 1, banned=p)), "n_banned")]
    for kw, word in more:
        rc, msg = _call_search(ens, **kw)
        assert rc != 0 and "beam_" in msg and word in msg, (word, rc, msg)
    # the workspace: at least the members' plain searches, the combined logits and one step of the other members' maps
    one = [lib.sat_beam_search_history_workspace_bytes(C.pointer(ens.dims[0].contents), K, 0, S), lib.sat_beam_search_workspace_bytes(C.pointer(ens.dims[1].contents), K)]
    got = lib.sat_beam_search_ensemble_workspace_bytes(C.byref(ens), K, S)
    extra = 2 * K * V * 4 + 2 * K * 6 * 4
    assert sum(one) + extra <= got <= sum(one) + extra + 2 * 256
    assert lib.sat_beam_search_ensemble_workspace_bytes(C.byref(ens), 0, S) == 0 and "beamk" in lib.sat_last_error().decode()
    assert lib.sat_beam_search_ensemble_workspace_bytes(C.byref(ens), K, -1) == 0 and "max_gen_length" in lib.sat_last_error().decode()
    rc = lib.sat_beam_search_ensemble(C.byref(ens), K, S, (C.c_float * 1)(1.0), 1, (C.c_int32 * 4)(1, 0, 2, 3), None, None, p, p, p, p, p, p, p, p, p, one[1], None)
    assert rc != 0 and "workspace" in lib.sat_last_error().decode()

    # sat_beam_ensemble_scores
    def scores(members=2, weights=(0.5, 0.5), combine=0, rows=5, v=V, T=1.0, logits=(p, p), out=p):
        arr = (C.c_void_p * max(len(logits), 1))(*logits) if logits is not None else None
        wts = (C.c_float * max(len(weights), 1))(*weights) if weights is not None else None
        rc = lib.sat_beam_ensemble_scores(arr, wts, members, combine, rows, v, T, out, None)
        return rc, lib.sat_last_error().decode()
    bad = [(dict(members=0), "members"), (dict(members=9), "members"), (dict(weights=(0.5, -0.5)), "weight[1]"), (dict(weights=(0.3, 0.3)), "sum"),
           (dict(weights=(float("nan"), 0.5)), "weight[0]"), (dict(combine=7), "combine"), (dict(rows=0), "rows"), (dict(v=0), "V="), (dict(T=0.0), "temperature"),
           (dict(T=-1.0), "temperature"), (dict(logits=(p, None)), "member 1"), (dict(logits=None), "null pointer"), (dict(weights=None), "null pointer"),
           (dict(out=None), "null pointer")]
    for kw, word in bad:
        rc, msg = scores(**kw)
        assert rc != 0 and "beam_ensemble_scores" in msg and word in msg, (word, rc, msg)
