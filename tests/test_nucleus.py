"""CPU: nucleus (top-p) sampling ("Sampled decoding").  The float64 restatement the GPU tests compare against is itself
checked against a brute-force definition and hand cases; the per-image host path's torch statement agrees with it; the C ABI keeps
the layout of sat_beam_sampling; the entry points and the Python surface refuse bad arguments before anything is launched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nucleus_ref as NR

V, K, S = 83, 4, 9


def _brute(row, topp):
    """the smallest leading run of the (score descending, id ascending) order whose mass reaches topp of the total"""
    ids = [v for v in range(len(row)) if math.isfinite(row[v])]
    if not ids:
        return []
    ids.sort(key=lambda v: (-row[v], v))
    mx = max(row[v] for v in ids)
    w = np.array([math.exp(row[v] - mx) for v in ids], dtype=np.float64)
    cum = np.cumsum(w)                                   # the running sum in sorted order, float64
    for n in range(1, len(ids) + 1):
        if topp < 1.0 and cum[n - 1] >= topp * cum[-1]:
            return sorted(ids[:n])
    return sorted(ids)


def test_restatement_equals_the_brute_force_definition():
    rs = np.random.RandomState(17)
    for trial in range(400):
        n = int(rs.randint(1, 13))
        row = rs.normal(0.0, 2.0, n)
        if trial % 3 == 0:                               # ties and holes
            row = np.round(row)
        if trial % 4 == 0:
            row[rs.randint(n)] = -np.inf
        topp = float(rs.choice([0.05, 0.3, 0.5, 0.8, 0.9, 0.99, 1.0]))
        got = NR.nucleus(row, topp)
        assert got == _brute(list(row), topp), (trial, row, topp)
        if np.isfinite(row).any():
            assert len(got) >= 1 and all(np.isfinite(row[v]) for v in got)
        assert NR.boundary_margin(row, topp) >= 0.0


def test_hand_cases():
    ninf = -np.inf
    one_hot = np.full(9, ninf); one_hot[4] = 0.0
    assert NR.nucleus(one_hot, 0.3) == [4] and NR.nucleus(one_hot, 1.0) == [4]
    dominant = np.log(np.array([0.01, 0.02, 0.9, 0.03, 0.04]))
    assert NR.nucleus(dominant, 0.5) == [2]
    for n, topp in [(10, 0.55), (10, 0.5), (7, 0.9), (64, 0.05), (5, 0.01)]:
        assert NR.nucleus(np.full(n, -1.5), topp) == list(range(math.ceil(topp * n))), (n, topp)
    row = np.array([0.3, ninf, -2.0, 1.0, ninf, -7.0])
    assert NR.nucleus(row, 1.0) == [0, 2, 3, 5]
    assert NR.nucleus(row, 1e-6) == [3]
    assert all(v not in NR.nucleus(row, p) for v in (1, 4) for p in (0.1, 0.5, 0.9, 0.999, 1.0))
    assert NR.nucleus(np.array([ninf, -3.0, ninf]), 0.4) == [1]
    assert NR.nucleus(np.full(4, ninf), 0.4) == []
    # a leader and a run of equal words with the cut inside the run: the leader and the four lowest tied ids
    shares = np.log(np.array([0.1, 0.1, 0.1, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1]))
    assert NR.nucleus(shares, 0.55) == [0, 1, 2, 3, 4]
    # the margin: the run counts as one position, 0.2 before it and 1.0 after it
    assert abs(NR.boundary_margin(shares, 0.55) - 0.35) < 1e-12
    assert abs(NR.boundary_margin(np.log(np.array([0.5, 0.3, 0.2])), 0.6) - 0.1) < 1e-12
    assert NR.boundary_margin(shares, 1.0) == float("inf")


def test_host_path_candidates_agree_with_the_restatement():
    """model.nucleus_candidates (the torch statement the per-image loop draws from): members, their order and the margin"""
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    rs = np.random.RandomState(5)
    rows = rs.normal(0.0, 2.5, (40, 31)).astype(np.float32)
    rows[::3] = np.round(rows[::3])                      # ties
    rows[1, :] = -np.inf; rows[1, 7] = 0.25              # a single finite entry
    rows[2, ::5] = -np.inf
    rows[4, :] = -np.inf                                 # no finite entry
    t = torch.from_numpy(rows)
    for topp in (0.05, 0.6, 0.95, 1.0):
        cand, margins = M.nucleus_candidates(t, topp, with_margin=True)
        cand = cand.tolist()
        for r in range(rows.shape[0]):
            mine = [c - r * 31 for c in cand if c // 31 == r]
            want = NR.nucleus(rows[r], topp)
            assert sorted(mine) == want, (r, topp)
            assert mine == sorted(mine, key=lambda v: (-rows[r, v], v))      # stable (-score, id) order
            m = NR.boundary_margin(rows[r], topp)
            assert margins[r] == m or abs(margins[r] - m) < 1e-12, (r, topp, margins[r], m)
        assert cand == sorted(cand, key=lambda c: c // 31)                   # rows in order
        assert torch.equal(M.nucleus_candidates(t, topp), torch.tensor(cand))


def test_sampling_struct_keeps_its_layout():
    """sample_topp took a reserved word: size 40 and normals at offset 32, as built at the parent commit"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    assert C.sizeof(L.BeamSampling) == 40
    assert L.BeamSampling.normals.offset == 32
    assert L.BeamSampling.sample_topp.offset == 28 and L.BeamSampling.sample_topp.size == 4
    assert L.BeamSampling.decoder_noise.offset == 24 and L.BeamSampling.gumbel.offset == 16
    unset = L.BeamSampling(method=2, sample_topk=3, seed=1)
    assert bytes(unset)[28:32] == b"\0\0\0\0"           # callers that never heard of the field pass zero bits
    assert L.SAMPLE_METHODS["nucleus"] == 3


def _decoder():
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    hp = O.default_hparams(vocab_size=V, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(3)
    return M.SATDecoder(hp).eval(), hp


def _search(dec, hp, entry, topp, con=None, gumbel=None, ws_ok=True):
    """sat_beam_search_sampled / _constrained with method 3 on host pointers: the checks run before the first launch, nothing is dereferenced"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    dims = Dk.decoder_dims(2, K, 2, 12, 32, 16, 24, 40, V, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    w, keep = dec._params_struct()
    ws_bytes = lib.sat_beam_search_constrained_workspace_bytes(C.byref(dims), K, 0)
    assert ws_bytes > 0
    p = torch.zeros(64, dtype=torch.int32).data_ptr()
    temps = (C.c_float * 1)(1.0)
    ids = (C.c_int32 * 4)(*[int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    smp = L.BeamSampling(method=3, sample_topk=3, seed=1, sample_topp=topp, gumbel=gumbel)
    tail = (p, p, p, p, p, p, p, p, p if ws_ok is not None else None, ws_bytes if ws_ok else 16, None)
    if entry == "sampled":
        rc = lib.sat_beam_search_sampled(C.byref(dims), C.byref(w), p, K, S, temps, 1, ids, C.byref(smp), *tail)
    else:
        rc = lib.sat_beam_search_constrained(C.byref(dims), C.byref(w), p, K, S, temps, 1, ids, C.byref(smp), C.byref(con) if con is not None else None, *tail)
    return rc, lib.sat_last_error().decode()


def test_search_entry_points_refuse_a_bad_topp_before_any_launch():
    from sat_amd import _lib as L
    dec, hp = _decoder()
    some = torch.zeros(8, dtype=torch.int32).data_ptr()
    for entry in ("sampled", "constrained"):
        for topp in (0.0, -0.1, 1.5, float("nan"), float("inf")):
            rc, msg = _search(dec, hp, entry, topp)
            assert rc != 0 and "sample_topp" in msg, (entry, topp, rc, msg)
        # a Gumbel table does not get past a null or a short workspace
        rc, msg = _search(dec, hp, entry, 0.9, gumbel=some, ws_ok=None)
        assert rc != 0 and "null pointer" in msg, (entry, rc, msg)
        rc, msg = _search(dec, hp, entry, 0.9, gumbel=some, ws_ok=False)
        assert rc != 0 and "workspace" in msg, (entry, rc, msg)
    # a constraint that is present (a banned id) does not change the answer; top-g does not combine with a sampling method
    rc, msg = _search(dec, hp, "constrained", 1.5, con=L.BeamConstraints(n_banned=1, banned=some))
    assert rc != 0 and "sample_topp" in msg, (rc, msg)
    rc, msg = _search(dec, hp, "constrained", 0.9, con=L.BeamConstraints(topg=2))
    assert rc != 0 and "beam_constrained" in msg and "sampling" in msg, (rc, msg)


def test_nucleus_keys_entry_point_refuses_bad_arguments_before_any_launch():
    from sat_amd import _lib as L
    lib = L.lib()
    p = torch.zeros(64, dtype=torch.float32).data_ptr()

    def call(rows=2, V_=8, topp=0.5, step=1.0, scores=p, keys=p):
        rc = lib.sat_nucleus_keys(scores, rows, V_, topp, step, 1, 1, None, keys, None, None)
        return rc, lib.sat_last_error().decode()

    for kw, word in [(dict(rows=0), "rows"), (dict(rows=-3), "rows"), (dict(V_=0), "V="), (dict(V_=-1), "V="),
                     (dict(topp=0.0), "topp"), (dict(topp=-0.1), "topp"), (dict(topp=1.5), "topp"), (dict(topp=float("nan")), "topp"),
                     (dict(step=0.0), "step"), (dict(scores=None), "null pointer"), (dict(keys=None), "null pointer")]:
        rc, msg = call(**kw)
        assert rc != 0 and "nucleus_keys" in msg and word in msg, (kw, rc, msg)


def test_python_surface():
    """topg with "nucleus" is the existing ValueError; a bad sample_topp is a ValueError; a CPU model gets as far as the library's
    "no GPU" error, so the method name is accepted everywhere"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, constraints, evaluation as E, model as M
    from oracle import sat_oracle as O
    dec, hp = _decoder()
    ann = torch.zeros(3, 12, 32)
    with pytest.raises(ValueError, match="topg"):
        constraints.resolve(hp.vocab_stoi, V, 3, K, S, "nucleus", topg=2)
    for fn in (dec.beam_decode, dec.beam_decode_batched):
        with pytest.raises(ValueError, match="topg"):
            fn(ann, (3, 4), beamk=K, max_gen_length=S, sample_method="nucleus", topg=2)
        for topp in (0.0, -0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="sample_topp"):
                fn(ann, (3, 4), beamk=K, max_gen_length=S, sample_method="nucleus", sample_topp=topp)
        with pytest.raises(L.SatHipError):
            fn(ann, (3, 4), beamk=K, max_gen_length=S, sample_method="nucleus", sample_topp=0.9)
        with pytest.raises(L.SatHipError):
            fn(ann, (3, 4), beamk=K, max_gen_length=S, sample_method="nucleus", sample_topp=1.0, prefix=[5], no_unk=True, banned=[7])
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over)))
    img = torch.zeros(2, 3, 64, 64)
    caps, lens = torch.zeros(2, 3, 9, dtype=torch.int64), torch.full((2, 3), 4)
    with pytest.raises(ValueError, match="topg"):
        model.forward(img, sample_method="nucleus", topg=2)
    with pytest.raises(ValueError, match="topg"):
        model.caption(img, sample_method="nucleus", topg=2, sample_topp=0.5)
    with pytest.raises(ValueError, match="topg"):
        model.val_batch_stats((img, caps, lens), sample_method="nucleus", topg=2)
    with pytest.raises(ValueError, match="topg"):
        E.caption_tokens(model, img, sample_method="nucleus", topg=2)
    with pytest.raises(ValueError, match="sample_topp"):
        model.caption(img, sample_method="nucleus", sample_topp=0.0)
    with pytest.raises(L.SatHipError):
        model.caption(img, beamk=3, sample_method="nucleus", sample_topp=0.9)


def test_notebook_search_space_is_unchanged():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    assert E.NOTEBOOK_SPACE["sample_methods"] == ["beam", "multinomial"]
    assert "sample_topp" not in E.draw_decode_params(np.random.RandomState(1))
