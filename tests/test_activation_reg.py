"""CPU: activation regularisation ("Activation regularisation").  The float64 specification (tests/activation_reg_ref.py)
equals Merity et al.'s plain means at equal lengths and its closed-form gradient is autograd's; the restated decode loop is the oracle's,
bit for bit; the new symbols are declared, exported and bound and the ABI version stays 23; every argument fault answers through the C ABI
before anything is launched; the two hparams are checked at construction."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import activation_reg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd")
NEW_SYMBOLS = ("sat_activation_reg_scratch_bytes", "sat_activation_reg_fwd", "sat_activation_reg_bwd", "sat_decoder_train_reg_fwd",
               "sat_decoder_train_bwd_reg")


def test_equal_lengths_are_the_plain_means():
    g = torch.Generator().manual_seed(1)
    T1, N, n = 6, 3, 8
    h = torch.randn(T1, N, n, generator=g, dtype=torch.float64)
    ar, tar, P, Q = R.reg_terms(h, [T1] * N)
    assert (P, Q) == (T1 * N, (T1 - 1) * N)
    assert abs(float(ar) - float(h.pow(2).mean())) <= 1e-15
    assert abs(float(tar) - float((h[1:] - h[:-1]).pow(2).mean())) <= 1e-15


def test_closed_form_gradient_is_autograds():
    g = torch.Generator().manual_seed(2)
    lengths = [5, 1, 3, 0]
    h = torch.randn(5, 4, 7, generator=g, dtype=torch.float64)
    ha = h.clone().requires_grad_()
    ar, tar, P, Q = R.reg_terms(ha, lengths)
    assert (P, Q) == (9, 6)
    g0, g1 = 1.7, -0.6
    (g0 * ar + g1 * tar).backward()
    ref = R.reg_grad(h, lengths, g0, g1)
    assert float((ref - ha.grad).abs().max()) <= 1e-15
    live = R.live_mask(lengths, 5)
    assert bool((ref[~live] == 0).all()) and bool((ha.grad[~live] == 0).all())
    # rows that are not live take no part, whatever they hold
    hn = h.clone(); hn[~live] = float("nan")
    ar2, tar2, _, _ = R.reg_terms(hn, lengths)
    assert float(ar2) == float(ar.detach()) and float(tar2) == float(tar.detach())
    assert torch.equal(R.reg_grad(hn, lengths, g0, g1), ref)
    mag = R.reg_grad_magnitude(h, lengths, g0, g1)
    assert bool((ref.abs() <= mag * (1 + 1e-12)).all())


def test_all_lengths_at_most_one_have_no_tar():
    h = torch.randn(3, 4, 5, dtype=torch.float64)
    ar, tar, P, Q = R.reg_terms(h, [1, 0, 1, 1])
    assert (P, Q) == (3, 0) and float(tar) == 0.0 and float(ar) > 0.0
    ar, tar, P, Q = R.reg_terms(h, [0, 0, 0, 0])
    assert (P, Q) == (0, 0) and float(ar) == 0.0 and float(tar) == 0.0


@pytest.mark.parametrize("eps,layers", [(1.0, 1), (0.0, 1), (0.0, 2)])
def test_restated_decode_loop_is_the_oracles(eps, layers):
    from oracle import prng, sat_oracle as O
    hp = O.default_hparams(encoder_dim=12, embed_dim=10, attention_dim=6, decoder_dim=14, vocab_size=40, decoder_layers=layers)
    sd = O.random_decoder_state(hp, 3)
    B, Rr, T = 3, 2, 8
    ann = torch.from_numpy(prng.uniform((B, hp.encoder_dim, 2, 3), 9, -1.0, 1.0))
    caps, lengths = prng.captions(B, Rr, T, hp.vocab_size, 10)
    caps, lengths = torch.from_numpy(caps), torch.from_numpy(lengths)
    draws = [0.9, 0.1, 0.7, 0.3, 0.8, 0.2, 0.6, 0.4]
    with torch.no_grad():
        a = O.decode_train(sd, hp, ann, caps, lengths, eps, draw=iter(draws).__next__)
        b = R.decode_train_hidden(sd, hp, ann, caps, lengths, eps, draw=iter(draws).__next__)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["alphas"], b["alphas"])
    assert b["hidden"].shape == (T - 1, B * Rr, hp.decoder_dim)
    ar, tar, P, Q = R.reg_terms(b["hidden"].double(), b["lengths"])
    assert P == int(lengths.sum()) and 0 < Q < P and float(ar) > 0 and float(tar) > 0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libsat_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_declared_and_bound(lib):
    from sat_amd import _lib, decoder as Dk
    raw = C.CDLL(os.path.join(PKG, "libsat_hip.so"))
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in _lib.SYMBOLS and ("%s(" % name) in header, name
    assert "#define SAT_HIP_ABI_VERSION 23" in header and lib.sat_abi_version() == 23       # symbols were added, nothing existing changed
    assert hasattr(Dk, "DecoderTrainRegFn")
    assert lib.sat_activation_reg_scratch_bytes(640, 21, 512) >= 16 and lib.sat_activation_reg_scratch_bytes(640, 21, 512) % 8 == 0
    assert lib.sat_activation_reg_scratch_bytes(0, 21, 512) == 0 and b"activation_reg_scratch_bytes" in lib.sat_last_error()


def test_activation_reg_argument_checks(lib):
    """every listed argument fault returns SAT_EINVAL (1) with a text that names the function; every check comes before the launch, so no
    GPU is touched"""
    p = 4096                                                                     # a non-null address: never dereferenced on the host
    fwd_names = ("hidden", "lengths", "N", "T1", "n", "P", "Q", "scratch", "out")
    bwd_names = ("hidden", "lengths", "N", "T1", "n", "P", "Q", "gscale", "dH")
    default = dict(hidden=p, lengths=p, N=5, T1=4, n=7, P=10, Q=6, scratch=p, out=p, gscale=p, dH=p)

    def fwd(**kw):
        return lib.sat_activation_reg_fwd(*[kw.get(k, default[k]) for k in fwd_names], None), lib.sat_last_error().decode()

    def bwd(**kw):
        return lib.sat_activation_reg_bwd(*[kw.get(k, default[k]) for k in bwd_names], None), lib.sat_last_error().decode()

    for call, what, nulls in ((fwd, "activation_reg_fwd", ("hidden", "lengths", "scratch", "out")),
                              (bwd, "activation_reg_bwd", ("hidden", "lengths", "gscale", "dH"))):
        for null in nulls:
            rc, msg = call(**{null: None})
            assert rc == 1 and what in msg and "null pointer" in msg and null in msg, (null, rc, msg)
        for kw, word in [(dict(N=0), "N=0"), (dict(N=-3), "N=-3"), (dict(T1=0), "T1=0"), (dict(T1=-1), "T1=-1"), (dict(n=0), "n=0"), (dict(n=-8), "n=-8"),
                         (dict(P=-1), "P=-1"), (dict(Q=-1), "Q=-1"), (dict(P=4, Q=5), "Q=5"), (dict(P=21, Q=6), "P=21")]:
            rc, msg = call(**kw)
            assert rc == 1 and what in msg and word in msg, (kw, rc, msg)


def test_decoder_train_reg_entries_check_their_arguments(lib):
    import numpy as np
    from sat_amd import _lib as L
    dims = L.DecoderDims(B=2, R=2, T=5, L=4, D=8, A=8, m=8, n=8, V=16, P=16, deep_output=1, padding_idx=0, layers=1)
    ws_bytes = lib.sat_decoder_workspace_bytes(C.byref(dims))
    some = 4096
    w = L.DecoderParams(**{k: some for k in L.PARAM_FIELDS})
    host = np.zeros(8, np.int32)
    batch = L.DecoderBatch(ann=some, caps=some, lengths=some, prow=some, src_row=some, step_offsets_host=host.ctypes.data, teacher_host=host.ctypes.data)
    for kw in (dict(workspace=None), dict(scratch=None), dict(out=None)):
        a = dict(workspace=some, scratch=some, out=some); a.update(kw)
        assert lib.sat_decoder_train_reg_fwd(C.byref(dims), C.byref(batch), a["workspace"], ws_bytes, a["scratch"], a["out"], None) == 1
        assert b"decoder_train_reg_fwd" in lib.sat_last_error() and b"null" in lib.sat_last_error()
    assert lib.sat_decoder_train_reg_fwd(C.byref(dims), C.byref(batch), some, ws_bytes - 256, some, some, None) == 1
    assert b"decoder_train_reg_fwd" in lib.sat_last_error() and b"workspace" in lib.sat_last_error()
    assert lib.sat_decoder_train_reg_fwd(None, C.byref(batch), some, ws_bytes, some, some, None) != 0
    args = (C.byref(dims), C.byref(w), C.byref(batch), some, some, some, C.byref(w), some, some, ws_bytes)
    assert lib.sat_decoder_train_bwd_reg(*args, C.c_void_p(4096), None, None, some) != 0
    assert b"decoder_train_bwd_reg" in lib.sat_last_error() and b"side stream and event" in lib.sat_last_error()
    assert lib.sat_decoder_train_bwd_reg(*args, C.c_void_p(4096), None, None, None) != 0          # NULL gscale: sat_decoder_train_bwd_fork's own refusal
    assert b"decoder_train_bwd_fork" in lib.sat_last_error()
    assert lib.sat_decoder_train_bwd_reg(*args[:-1], ws_bytes - (32 << 20), None, None, None, some) != 0
    assert b"decoder_train_bwd_reg" in lib.sat_last_error() and b"workspace" in lib.sat_last_error()


def _hparams(**over):
    from oracle import sat_oracle as O
    base = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    base.update(over)
    return vars(O.default_hparams(**base))


def test_hparams_are_checked_at_construction_and_default_to_zero():
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    torch.manual_seed(5)
    m = M.SAT(**_hparams())
    assert m.hp.ar_alpha == 0.0 and m.hp.tar_beta == 0.0 and m.reg_coefficients() == (0.0, 0.0)
    m = M.SAT(**_hparams(ar_alpha=2.0, tar_beta=1.0, opt="asgd"))
    assert m.reg_coefficients() == (2.0, 1.0)
    for kw in (dict(ar_alpha=-1), dict(tar_beta=float("nan")), dict(ar_alpha=float("inf")), dict(tar_beta=-0.5), dict(ar_alpha="2")):
        with pytest.raises(ValueError, match="ar_alpha|tar_beta"):
            M.SAT(**_hparams(**kw))
