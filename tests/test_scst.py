"""CPU: self-critical sequence training ("Self-critical training").  The float64 specification the GPU tests compare against
(tests/scst_ref.py) is checked against torch autograd and by hand; the three new symbols are exported, declared and bound while the ABI
version stays 23; every SAT_EINVAL path answers through the C ABI before anything is launched; the Python surface raises ValueError
before it touches the GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import scst_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd")
NEW_SYMBOLS = ("sat_policy_nll_fwd", "sat_policy_nll_bwd", "sat_scst_prepare")


def _rows(P, V, seed):
    from oracle import prng
    logits = torch.from_numpy(prng.uniform((P, V), seed, -4.0, 4.0).astype(np.float64))
    targets = torch.from_numpy(prng.integers((P,), seed + 1, 4, V))              # ids 0..3 are the masked ones here
    weight = torch.from_numpy(prng.uniform((P,), seed + 2, -2.0, 2.0).astype(np.float64))
    return logits, targets, weight


@pytest.mark.parametrize("n_first", [0, 2, 6])
@pytest.mark.parametrize("inv_t", [1.0, 1 / 0.7])
def test_reference_gradient_is_autograd_of_its_own_loss(n_first, inv_t):
    logits, targets, weight = _rows(6, 23, 11)
    weight[1] = 0.0
    ids = (2, 0, 3, 1)
    x = logits.clone().requires_grad_()
    loss, logq, lse = R.policy_loss(x, targets, weight, inv_t, ids, n_first, 0.37)
    (2.5 * loss).backward()
    logq, lse = logq.detach(), lse.detach()
    want = R.policy_grad(logits, targets, weight, inv_t, ids, n_first, 0.37, g=2.5)
    assert torch.allclose(x.grad, want, rtol=0, atol=1e-14)
    keep = R.unmasked(6, 23, ids, n_first)
    assert bool((want[~keep] == 0).all()) and bool((want[1] == 0).all())
    assert int((~keep).sum()) == 4 * n_first + 2 * (6 - n_first)
    # the distribution is the softmax renormalised over the unmasked words: the probabilities of every row sum to one there
    q = torch.exp(logits * inv_t - lse[:, None]) * keep
    assert torch.allclose(q.sum(1), torch.ones(6, dtype=torch.float64), atol=1e-13)
    # by hand for row 0
    row = [float(logits[0, v]) * inv_t for v in range(23) if keep[0, v]]
    lse0 = math.log(sum(math.exp(v) for v in row))
    assert abs(float(lse[0]) - lse0) < 1e-12 and abs(float(logq[0]) - (float(logits[0, targets[0]]) * inv_t - lse0)) < 1e-12


def test_reference_bad_targets_and_zero_rows():
    logits, targets, weight = _rows(4, 9, 5)
    ids = (0, 1, 2, 3)
    for bad, n_first in ((-1, 0), (9, 0), (1, 0), (3, 4)):
        t = targets.clone(); t[2] = bad
        loss, logq, _ = R.policy_loss(logits, t, weight, 1.0, ids, n_first, 1.0)
        assert math.isnan(float(loss)) and math.isnan(float(logq[2])) and not math.isnan(float(logq[0]))
        w0 = weight.clone(); w0[2] = 0.0                                         # a row of weight zero adds exactly 0, whatever it holds
        loss, _, _ = R.policy_loss(logits, t, w0, 1.0, ids, n_first, 1.0)
        assert math.isfinite(float(loss))
        assert bool(torch.isfinite(R.policy_grad(logits, t, weight, 1.0, ids, n_first, 1.0)).all())
    t = targets.clone(); t[2] = 3                                                # masked at the first step only
    assert math.isfinite(float(R.policy_loss(logits, t, weight, 1.0, ids, 2, 1.0)[0]))
    assert float(R.policy_loss(logits, targets, torch.zeros(4, dtype=torch.float64), 1.0, ids, 0, 1.0)[0]) == 0.0


def test_reference_prepare_by_hand():
    S, K = 4, 2
    tok = np.array([[7, 8, 0, 0, 0], [5, 6, 7, 8, 0], [9, 0, 0, 0, 0], [4, 5, 0, 0, 0]], np.int32)
    ln = np.array([2, 4, 1, 2], np.int32)
    sc = np.array([[1.0, 0.5], [0.25, 0.5], [2.0, 0.0], [0.0, 1.0]])
    ids = (50, 0, 51, 49)
    o = R.prepare(tok, ln, sc, None, K, 1.0, 2.0, R.MEAN, ids)
    assert o["reward"].tolist() == [2.0, 1.25, 2.0, 2.0] and o["baseline"].tolist() == [1.25, 2.0, 2.0, 2.0]
    assert o["advantage"].tolist() == [0.75, -0.75, 0.0, 0.0]
    assert o["caps"].tolist() == [[50, 7, 8, 51, 0, 0], [50, 5, 6, 7, 8, 51], [50, 9, 51, 0, 0, 0], [50, 4, 5, 51, 0, 0]]
    assert o["lengths"].tolist() == [3, 5, 2, 3] and o["count"].tolist() == [3, 4, 2, 3]
    assert o["step_weight"].tolist() == [[0.75, 0.75, 0.75, 0, 0], [-0.75, -0.75, -0.75, -0.75, 0], [0] * 5, [0] * 5]
    g = R.prepare(tok, ln, sc, np.array([[0.5, 0.0], [3.0, 0.0]]), K, 1.0, 2.0, R.GREEDY, ids)
    assert g["baseline"].tolist() == [0.5, 0.5, 3.0, 3.0] and g["advantage"].tolist() == [1.5, 0.75, -1.0, -1.0]
    c = R.prepare(tok, np.array([0, 9, 1, 2]), sc, None, K, 1.0, 2.0, R.MEAN, ids)            # lengths clamped to [1, S]
    assert c["lengths"].tolist() == [2, 5, 2, 3] and c["caps"][0].tolist() == [50, 7, 51, 0, 0, 0]


def test_reference_ancestral_draw():
    logits = [0.0, 5.0, 1.0, 4.0, 9.0]
    word, gap = R.ancestral_draw(logits, 1.0, (4, 0), [0.0] * 5)
    assert word == 1 and abs(gap - 1.0) < 1e-12                                  # 9.0 is masked; 5.0 leads 4.0 by one
    word, _ = R.ancestral_draw(logits, 2.0, (4, 0), [0.0, 0.0, 3.0, 0.0, 100.0])
    assert word == 2                                                             # 1/2 + 3 beats 5/2; the masked word stays out whatever its G
    assert R.ancestral_draw([1.0, 2.0, 2.0], 1.0, (), [0.0, 0.0, 0.0])[0] == 1    # ties go to the lower id


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libsat_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_declared_and_bound(lib):
    from sat_amd import _lib, decoder as Dk, model as M, scst  # noqa: F401
    raw = C.CDLL(os.path.join(PKG, "libsat_hip.so"))
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in _lib.SYMBOLS and ("int %s(" % name) in header, name
    assert "#define SAT_SAMPLE_ANCESTRAL 4" in header and "#define SAT_HIP_ABI_VERSION 23" in header
    assert "#define SAT_SCST_BASELINE_GREEDY 0" in header and "#define SAT_SCST_BASELINE_MEAN 1" in header
    assert lib.sat_abi_version() == 23                                           # symbols were added, nothing existing changed
    assert _lib.SAMPLE_METHODS["ancestral"] == 4 and "ancestral" in M.SAMPLE_METHODS
    assert _lib.SAMPLE_METHODS == {"beam": 0, "multinomial": 1, "topk": 2, "nucleus": 3, "ancestral": 4}
    assert _lib.SCST_BASELINES == {"greedy": 0, "mean": 1} and scst.BASELINES == ("greedy", "mean")
    assert hasattr(Dk, "PolicyNLLFn") and hasattr(M.SAT, "scst_step")


def test_policy_loss_argument_checks(lib):
    """null pointers, empty sizes, n_first_rows outside [0, P] and a temperature that is not positive and finite return SAT_EINVAL (1) with
    text from both entry points; every check comes before the launch, so no GPU is touched"""
    p = 4096                                                                     # a non-null address: never dereferenced on the host
    fwd_names = ("logits", "targets", "weight", "P", "V", "inv_t", "ids", "n_first", "scale", "lse", "logq", "out")
    bwd_names = ("logits", "targets", "weight", "lse", "P", "V", "inv_t", "ids", "n_first", "scale", "gscale", "dlogits")
    default = dict(logits=p, targets=p, weight=p, P=6, V=40, inv_t=1.0, ids=p, n_first=2, scale=0.5, lse=p, logq=p, out=p, gscale=None, dlogits=p)

    def fwd(**kw):
        return lib.sat_policy_nll_fwd(*[kw.get(n, default[n]) for n in fwd_names], None), lib.sat_last_error().decode()

    def bwd(**kw):
        return lib.sat_policy_nll_bwd(*[kw.get(n, default[n]) for n in bwd_names], None), lib.sat_last_error().decode()

    for call, what, nulls in ((fwd, "policy_nll_fwd", ("logits", "targets", "weight", "ids", "lse", "logq", "out")),
                              (bwd, "policy_nll_bwd", ("logits", "targets", "weight", "lse", "ids", "dlogits"))):
        for null in nulls:
            rc, msg = call(**{null: None})
            assert rc == 1 and what in msg and "null pointer" in msg, (null, rc, msg)
        for kw, word in [(dict(P=0), "P=0"), (dict(P=-2), "P=-2"), (dict(V=0), "V=0"), (dict(V=-1), "V=-1"), (dict(n_first=-1), "n_first_rows"),
                         (dict(n_first=7), "n_first_rows"), (dict(inv_t=0.0), "inv_temperature"), (dict(inv_t=-1.0), "inv_temperature"),
                         (dict(inv_t=float("inf")), "inv_temperature"), (dict(inv_t=float("nan")), "inv_temperature"),
                         (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale")]:
            rc, msg = call(**kw)
            assert rc == 1 and what in msg and word in msg, (kw, rc, msg)


def test_scst_prepare_argument_checks(lib):
    from sat_amd import _lib
    p = 4096
    ids = (C.c_int32 * 4)(58, 0, 59, 57)
    names = ("tok", "len", "scores", "greedy", "B", "K", "S", "wc", "wr", "mode", "ids", "reward", "baseline", "adv", "caps", "lengths", "sw", "count")
    default = dict(tok=p, len=p, scores=p, greedy=None, B=2, K=3, S=5, wc=1.0, wr=0.0, mode=1, ids=ids, reward=p, baseline=None, adv=p, caps=p,
                   lengths=p, sw=p, count=p)

    def call(**kw):
        return lib.sat_scst_prepare(*[kw.get(n, default[n]) for n in names], None), lib.sat_last_error().decode()

    for null in ("tok", "len", "scores", "ids", "reward", "adv", "caps", "lengths", "sw", "count"):
        rc, msg = call(**{null: None})
        assert rc == 1 and "scst_prepare" in msg and "null pointer" in msg, (null, rc, msg)
    for kw, word in [(dict(B=0), "non-positive"), (dict(K=0), "non-positive"), (dict(S=0), "non-positive"), (dict(B=-1), "non-positive"),
                     (dict(K=_lib.SCST_MAX_SAMPLES + 1), "over the limits"), (dict(S=_lib.CAPTION_MAX_LEN), "over the limits"),
                     (dict(mode=2), "baseline mode"), (dict(mode=-1), "baseline mode"), (dict(mode=0), "scores_greedy"),
                     (dict(K=1), "K >= 2"), (dict(wc=float("nan")), "not finite"), (dict(wr=float("inf")), "not finite")]:
        rc, msg = call(**kw)
        assert rc == 1 and "scst_prepare" in msg and word in msg, (kw, rc, msg)


def _decoder(V=83):
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    hp = O.default_hparams(vocab_size=V, encoder_dim=32, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(3)
    return M.SATDecoder(hp).eval(), hp


def _search(dec, hp, K, con=None, entry="sampled", method=4):
    """method 4 through the search entry points on host pointers: the checks run before the first launch, nothing is dereferenced"""
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    dims = Dk.decoder_dims(2, K, 2, 12, 32, 16, 24, 40, 83, 0, hp.deep_output, dec.pad_idx, 0, layers=1)
    w, keep = dec._params_struct()
    ws_bytes = lib.sat_beam_search_constrained_workspace_bytes(C.byref(dims), K, 0)
    p = torch.zeros(64, dtype=torch.int32).data_ptr()
    temps = (C.c_float * 1)(1.0)
    ids = (C.c_int32 * 4)(*[int(hp.vocab_stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    smp = L.BeamSampling(method=method, sample_topk=3, seed=1)
    tail = (p, p, p, p, p, p, p, p, p, ws_bytes, None)
    if entry == "sampled":
        rc = lib.sat_beam_search_sampled(C.byref(dims), C.byref(w), p, K, 6, temps, 1, ids, C.byref(smp), *tail)
    else:
        rc = lib.sat_beam_search_constrained(C.byref(dims), C.byref(w), p, K, 6, temps, 1, ids, C.byref(smp), C.byref(con), *tail)
    return rc, lib.sat_last_error().decode()


def test_search_refuses_ancestral_with_a_beam_or_a_constraint_before_any_launch(lib):
    from sat_amd import _lib as L
    dec, hp = _decoder()
    some = torch.zeros(8, dtype=torch.int32).data_ptr()
    for K in (2, 5):
        rc, msg = _search(dec, hp, K)
        assert rc == 1 and "ancestral" in msg and "beamk" in msg, (K, rc, msg)
    for con in (L.BeamConstraints(n_banned=1, banned=some), L.BeamConstraints(max_prefix=1, prefix=some, prefix_len=some)):
        rc, msg = _search(dec, hp, 1, con=con, entry="constrained")
        assert rc == 1 and "ancestral" in msg and "constraints" in msg, (rc, msg)
    rc, msg = _search(dec, hp, 1, con=L.BeamConstraints(topg=2), entry="constrained")
    assert rc == 1, (rc, msg)
    rc, msg = _search(dec, hp, 1, method=5)                                       # the range check moved up by one, not away
    assert rc == 1 and "sampling method 5" in msg, (rc, msg)


def test_python_surface_refuses_before_any_launch():
    """every refusal is a ValueError raised on the host; a call that passes the checks on a CPU model gets as far as the library's "no GPU"
    error, so the method name is accepted everywhere it is listed"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, constraints, evaluation as E, model as M, scst
    from oracle import sat_oracle as O
    for kw in (dict(beamk=2), dict(beamk=3), dict(beamk=1, topg=2), dict(beamk=1, prefix=[5]), dict(beamk=1, banned=[7]), dict(beamk=1, no_unk=True),
               dict(beamk=1, graph=True)):
        with pytest.raises(ValueError, match="ancestral"):
            constraints.check_ancestral("ancestral", **kw)
    constraints.check_ancestral("ancestral", 1)
    constraints.check_ancestral("beam", 3, True, topg=2)                          # the other methods are not its business
    dec, hp = _decoder()
    ann = torch.zeros(3, 12, 32)
    with pytest.raises(ValueError, match="ancestral"):
        dec.beam_decode(ann, (3, 4), beamk=1, max_gen_length=6, sample_method="ancestral")
    for kw in (dict(beamk=2), dict(beamk=1, prefix=[5]), dict(beamk=1, no_unk=True), dict(beamk=1, graph=True)):
        with pytest.raises(ValueError, match="ancestral"):
            dec.beam_decode_batched(ann, (3, 4), max_gen_length=6, sample_method="ancestral", **kw)
    with pytest.raises(L.SatHipError):
        dec.beam_decode_batched(ann, (3, 4), beamk=1, max_gen_length=6, sample_method="ancestral")
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**over)))
    img = torch.zeros(2, 3, 64, 64)
    caps, lens = torch.zeros(2, 3, 9, dtype=torch.int64), torch.full((2, 3), 4)
    with pytest.raises(ValueError, match="ancestral"):
        model.forward(img, beamk=2, sample_method="ancestral")
    with pytest.raises(ValueError, match="ancestral"):
        model.forward(img, beamk=1, max_gen_length=0, sample_method="ancestral")
    with pytest.raises(ValueError, match="ancestral"):
        model.caption(img, sample_method="ancestral")                             # the default beam of 3
    with pytest.raises(ValueError, match="ancestral"):
        model.caption(img, beamk=1, sample_method="ancestral", banned=[4])
    with pytest.raises(ValueError, match="ancestral"):
        model.val_batch_stats((img, caps, lens), beamk=2, sample_method="ancestral")
    with pytest.raises(ValueError, match="ancestral"):
        E.caption_tokens(model, img, beamk=1, sample_method="ancestral", graph=True)
    model.__dict__["beam_graph"] = True
    with pytest.raises(ValueError, match="graph"):
        model.caption(img, beamk=1, sample_method="ancestral")
    model.__dict__["beam_graph"] = False
    with pytest.raises(L.SatHipError):
        model.caption(img, beamk=1, sample_method="ancestral")
    # scst_step: a missing or empty corpus, too few samples for the mean baseline, an unknown baseline, a vocabulary the reward cannot key
    corpus = E.ReferenceCorpus(60, device="cpu"); corpus.images = 5               # never allocated: no check may reach the device
    batch = (img, caps, lens)
    step0 = model.sat_global_step()
    for kw, word in [(dict(corpus=None), "ReferenceCorpus"), (dict(corpus=E.ReferenceCorpus(60, device="cpu")), "ReferenceCorpus"),
                     (dict(samples=1), "samples >= 2"), (dict(samples=0, baseline="greedy"), "samples"), (dict(baseline="median"), "baseline"),
                     (dict(samples=L.SCST_MAX_SAMPLES + 1), "samples"), (dict(max_gen_length=0), "max_gen_length"),
                     (dict(max_gen_length=L.CAPTION_MAX_LEN), "max_gen_length"), (dict(temperature=0.0), "temperature"),
                     (dict(temperature=[1.0, 0.5]), "temperature"), (dict(reward=(1.0,)), "reward"), (dict(reward=(1.0, float("nan"))), "reward")]:
        args = dict(corpus=corpus); args.update(kw)
        with pytest.raises(ValueError, match=word):
            model.scst_step(batch, **args)
    model.hp["vocab_size"] = E.MAX_VOCAB + 1
    with pytest.raises(ValueError, match="vocab_size"):
        model.scst_step(batch, corpus)
    model.hp["vocab_size"] = 60
    assert model.sat_global_step() == step0                                       # a refused step is no step
    with pytest.raises(L.SatHipError):
        model.scst_step(batch, corpus, samples=1, baseline="greedy")
    for kw, word in [(dict(baseline="mean", samples=1), "samples >= 2"), (dict(baseline="greedy", samples=2), "scores_greedy"),
                     (dict(baseline="other", samples=2), "baseline")]:
        with pytest.raises(ValueError, match=word):
            scst.prepare(torch.zeros(2, 4, dtype=torch.int32), torch.ones(2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.float64),
                         ids=(58, 0, 59, 57), **kw)
