"""CPU: the constrained search (forced prefix, top-g clipping, banned ids) refuses bad arguments before anything is launched -
the C entry point with a status and a message, the Python surface with the ValueErrors of DESIGN.md 5 "Constrained search" -
and evaluation.random_search keeps its columns unless the space asks for top-g."""
import ctypes as C

import numpy as np
import pytest
import torch

V, K, S = 83, 4, 9


def _decoder(**over):
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    hp = O.default_hparams(vocab_size=V, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40, **over)
    torch.manual_seed(3)
    return M.SATDecoder(hp).eval(), hp


def _call(dec, hp, con, method=0, sample_topk=3, mgl=S, B=2):
    """sat_beam_search_constrained on host pointers: every check under test runs before the first launch, nothing is dereferenced"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    dims = Dk.decoder_dims(B, K, 2, 12, 32, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    w, keep = dec._params_struct()
    ws_bytes = lib.sat_beam_search_constrained_workspace_bytes(C.byref(dims), K, max(0, min(V, con.topg)) if con is not None else 0)
    assert ws_bytes >= lib.sat_beam_search_workspace_bytes(C.byref(dims), K) > 0
    buf = torch.zeros(64, dtype=torch.int32)
    p = buf.data_ptr()
    temps = (C.c_float * 1)(1.0)
    ids = (C.c_int32 * 4)(*[int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    smp = L.BeamSampling(method=method, sample_topk=sample_topk, seed=1) if method else None
    rc = lib.sat_beam_search_constrained(C.byref(dims), C.byref(w), p, K, mgl, temps, 1, ids, C.byref(smp) if smp is not None else None,
                                         C.byref(con) if con is not None else None, p, p, p, p, p, p, p, p, p, ws_bytes, None)
    return rc, lib.sat_last_error().decode()


def test_entry_point_refuses_bad_constraints_before_any_launch():
    from sat_amd import _lib as L
    dec, hp = _decoder()
    some = torch.zeros(8, dtype=torch.int32).data_ptr()
    cases = [
        (L.BeamConstraints(topg=-1), 0, "topg"),
        (L.BeamConstraints(topg=V + 1), 0, "topg"),
        (L.BeamConstraints(topg=2), 1, "sampling"),                                                   # top-g with a sampling method
        (L.BeamConstraints(topg=2), 2, "sampling"),
        (L.BeamConstraints(max_prefix=S + 1, prefix=some, prefix_len=some), 0, "max_prefix"),
        (L.BeamConstraints(max_prefix=-1), 0, "max_prefix"),
        (L.BeamConstraints(max_prefix=2, prefix=None, prefix_len=some), 0, "null pointer"),
        (L.BeamConstraints(max_prefix=2, prefix=some, prefix_len=None), 0, "null pointer"),
        (L.BeamConstraints(n_banned=1, banned=None), 0, "null pointer"),
        (L.BeamConstraints(n_banned=-1), 0, "n_banned"),
    ]
    for con, method, word in cases:
        rc, msg = _call(dec, hp, con, method)
        assert rc != 0 and "beam_constrained" in msg and word in msg, (word, rc, msg)
    # the workspace query refuses what the search would refuse
    from sat_amd import decoder as Dk
    dims = Dk.decoder_dims(2, K, 2, 12, 32, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    lib = L.lib()
    assert lib.sat_beam_search_constrained_workspace_bytes(C.byref(dims), K, V + 1) == 0 and "topg" in lib.sat_last_error().decode()
    plain = lib.sat_beam_search_workspace_bytes(C.byref(dims), K)
    assert lib.sat_beam_search_constrained_workspace_bytes(C.byref(dims), K, 0) == plain
    assert lib.sat_beam_search_constrained_workspace_bytes(C.byref(dims), K, 3) >= plain + 2 * 2 * K * 3 * 4


def test_python_surface_raises_before_touching_a_gpu():
    """CPU annotations: a call that got past the checks would fail with SatHipError (no CPU fallback), so ValueError proves the order"""
    from sat_amd import _lib as L
    dec, hp = _decoder()
    ann = torch.zeros(3, 12, 32)
    stoi = hp.vocab_stoi
    bad = [
        dict(prefix=[5, int(stoi["<START>"])]), dict(prefix=[int(stoi["<PAD>"])]), dict(prefix=[[5], [int(stoi["<END>"])], []]),
        dict(prefix=[int(stoi["<UNK>"])]),
        dict(prefix=[7, 8], banned=[8]),                      # a banned id in a prefix
        dict(prefix=[7], no_unk=True, banned=[7]),
        dict(prefix=list(range(1, S + 2))),                   # P_b > S
        dict(prefix=[V]), dict(prefix=[-1]),
        dict(prefix=[[5], [6]]),                              # 2 prefixes for 3 images
        dict(banned=[int(stoi["<END>"])]), dict(banned=[V]), dict(banned=[-2]),
        dict(banned=list(range(1, V - 3 - (K - 1)))),         # K - 1 unmasked ids left
        dict(topg=7, banned=list(range(1, V - 3 - 6))),       # 6 left, topg 7
        dict(topg=0), dict(topg=V + 1),
        dict(topg=2, sample_method="multinomial"), dict(topg=2, sample_method="topk"),
    ]
    for kw in bad:
        for fn in (dec.beam_decode, dec.beam_decode_batched):
            with pytest.raises(ValueError):
                fn(ann, (3, 4), beamk=K, max_gen_length=S, **kw)
    # exactly K ids left is enough; the call then reaches the GPU check
    with pytest.raises(L.SatHipError):
        dec.beam_decode_batched(ann, (3, 4), beamk=K, max_gen_length=S, banned=list(range(1, V - 3 - K)))
    with pytest.raises(L.SatHipError):
        dec.beam_decode_batched(ann, (3, 4), beamk=K, max_gen_length=S, prefix=[[5], [6, 7], []], topg=2, no_unk=True)


def test_string_prefix_is_looked_up_in_the_vocabulary():
    from sat_amd import constraints
    _, hp = _decoder()
    stoi = dict(hp.vocab_stoi); stoi.update({"a": 4, "photo": 9, "of": 2})
    con = constraints.resolve(stoi, V, 3, K, S, prefix="a photo  of")
    assert con.prefix == [[4, 9, 2]] * 3 and con.max_prefix == 3 and con.topg == 0 and con.banned == []
    con = constraints.resolve(stoi, V, 2, K, S, prefix=["a photo", torch.tensor([9])], no_unk=True, topg=2)
    assert con.prefix == [[4, 9], [9]] and con.banned == [int(stoi["<UNK>"])] and con.topg == 2
    with pytest.raises(ValueError, match="zebra"):
        constraints.resolve(stoi, V, 3, K, S, prefix="a zebra")
    with pytest.raises(ValueError):
        constraints.resolve(stoi, V, 3, K, S, prefix="a <UNK>")
    assert constraints.resolve(stoi, V, 3, K, S) is None
    assert constraints.resolve(stoi, V, 3, K, S, prefix=[[], [], []]) is None        # nothing constrains: the plain search


def test_sat_surface_raises_before_the_encoder_runs():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, model as M, visualize as Z
    from oracle import sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over)))
    img = torch.zeros(2, 3, 64, 64)
    caps, lens = torch.zeros(2, 3, 9, dtype=torch.int64), torch.full((2, 3), 4)
    with pytest.raises(ValueError, match="zebra"):
        model.caption(img, prefix="zebra")
    with pytest.raises(ValueError):
        model.caption(img, topg=2, sample_method="topk")
    with pytest.raises(ValueError):
        model.val_batch((img, caps, lens), banned=[59])            # <END>
    with pytest.raises(ValueError):
        E.caption_tokens(model, img, prefix=[57])                  # <UNK>
    with pytest.raises(ValueError):
        model.val_batch_stats((img, caps, lens), topg=61)
    with pytest.raises(ValueError):
        E.evaluate(model, [(img, caps, lens)], topg=2, sample_method="multinomial")
    with pytest.raises(ValueError):
        Z.caption_image(model, [np.zeros((8, 8, 3), np.uint8)], prefix="zebra")
    with pytest.raises(ValueError):
        model.visualize([np.zeros((8, 8, 3), np.uint8)], no_unk=True, banned=list(range(1, 56)))


def test_random_search_columns_change_only_with_topgs():
    from sat_amd import evaluation as E
    assert "topgs" not in E.NOTEBOOK_SPACE and len(E.HEADERS) == 13 and "topg" not in E.HEADERS
    plain = [E.draw_decode_params(np.random.RandomState(7)) for _ in range(1)][0]
    assert list(plain) == E.HEADERS[:6]
    space = dict(E.NOTEBOOK_SPACE, topgs=[None, 2, 3])
    rs_a, rs_b = np.random.RandomState(11), np.random.RandomState(11)
    seen = set()
    for _ in range(40):
        row = E.draw_decode_params(rs_b, space)
        assert list(row) == E.HEADERS[:6] + ["topg"]
        assert row["topg"] in (None, 2, 3) and (row["sample_method"] == "beam" or row["topg"] is None)
        seen.add(row["topg"])
    assert seen == {None, 2, 3}
    first = E.draw_decode_params(rs_a, space)
    assert {k: first[k] for k in E.HEADERS[:6]} == E.draw_decode_params(np.random.RandomState(11))     # the notebook's draws come first, unchanged

    class Model:                                                   # random_search's rows: the columns of the trial plus the metrics
        def val_batch_stats(self, batch, **kw):
            self.seen.append(kw)
            return E.CaptionStats(torch.zeros(12, dtype=torch.int64), torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64), 1, None)
    m = Model(); m.seen = []
    rows = E.random_search(m, [None], 2, seed=3)
    assert all("topg" not in r for r in rows) and all("topg" not in kw for kw in m.seen)
    assert list(rows[0])[:13] == E.HEADERS
    rows = E.random_search(m, [None], 3, space=space, seed=3)
    assert all("topg" in r for r in rows) and all("topg" in kw for kw in m.seen[2:])
