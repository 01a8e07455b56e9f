"""CPU: weight-drop and variational dropout ("Weight-drop and variational dropout").  The two hyper-parameters are checked
at construction and default to off; ``sat_decoder_dims`` carries them at its end, so the keyword constructions of before zero-fill them;
the host replica of the weight-drop mask is ``dropout_scale_reference`` on stream 3 under the index formula of the kernels; the new
symbols are declared, exported and bound and every argument fault answers through the C ABI before anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sat_weight_drop", "sat_weight_drop_grad", "sat_decoder_pack_weights")
SAT_EINVAL = 1                                                 # csrc/common.h


def small_hparams(**over):
    from oracle import sat_oracle as O
    return O.default_hparams(**dict(dict(vocab_size=40, encoder_dim=16, embed_dim=12, attention_dim=8, decoder_dim=20), **over))


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), "0.5", True, None])
def test_weight_drop_outside_the_half_open_unit_interval_is_refused(bad):
    from sat_amd import model as M
    with pytest.raises(ValueError, match="weight_drop"):
        M.SATDecoder(small_hparams(weight_drop=bad))
    over = dict(vars(small_hparams(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=2)), weight_drop=bad)
    with pytest.raises(ValueError, match="weight_drop"):
        M.SAT(**over)


def test_defaults_are_off_and_the_reference_kwargs_still_construct():
    from sat_amd import model as M
    args = small_hparams(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=2)
    assert not hasattr(args, "weight_drop") and not hasattr(args, "variational_dropout")
    sat = M.SAT(**vars(args))
    assert sat.hp.weight_drop == 0.0 and sat.hp.variational_dropout is False
    assert sat.weight_drop_args() == (0.0, False)
    dec = M.SATDecoder(small_hparams())                       # a namespace without the two keys
    assert dec.weight_drop_args() == (0.0, False)
    dec = M.SATDecoder(small_hparams(weight_drop=0.5, variational_dropout=True))
    assert dec.weight_drop_args() == (0.5, True)
    with pytest.raises(ValueError, match="variational_dropout"):
        M.SATDecoder(small_hparams(variational_dropout="yes"))


def test_dropout_args_draw_a_seed_for_weight_drop_alone_and_stay_off_in_eval():
    from sat_amd import model as M
    dec = M.SATDecoder(small_hparams(weight_drop=0.5)).train()
    a = dec._dropout_args()
    assert a[:2] == (0.0, 0.0) and a[3:] == (0.5, False) and a[2] != dec._dropout_args()[2]      # a fresh seed per call
    assert dec._dropout_args(77) == (0.0, 0.0, 77, 0.5, False)
    assert dec.eval()._dropout_args(77) == (0.0, 0.0, 0)
    # variational dropout locks the masks of the two rates: without a rate there is nothing to lock, and today's 3-tuple stays
    dec = M.SATDecoder(small_hparams(variational_dropout=True)).train()
    assert dec._dropout_args(77) == (0.0, 0.0, 0)
    dec = M.SATDecoder(small_hparams(variational_dropout=True, dropout=0.3)).train()
    assert dec._dropout_args(77) == (0.3, 0.0, 77, 0.0, True)
    assert M.SATDecoder(small_hparams(dropout=0.3)).train()._dropout_args(77) == (0.3, 0.0, 77)


def test_decoder_dims_carries_the_two_fields_at_its_end():
    from sat_amd import _lib as L, decoder as Dk
    names = [f[0] for f in L.DecoderDims._fields_]
    assert names[-3:] == ["dropout_seed", "weight_drop", "variational_dropout"]
    assert L.DecoderDims.weight_drop.offset == L.DecoderDims.dropout_seed.offset + 8
    assert L.DecoderDims.variational_dropout.offset == L.DecoderDims.weight_drop.offset + 4
    assert C.sizeof(L.DecoderDims) == L.DecoderDims.variational_dropout.offset + 4
    d = L.DecoderDims(B=2, R=1, T=3, dropout=0.25, dropout_seed=9)              # a construction from before the fields existed
    assert d.weight_drop == 0.0 and d.variational_dropout == 0
    d = Dk.decoder_dims(2, 3, 9, 6, 16, 8, 12, 20, 40, 11, True, 0, 0, 0.0, 0.3, 0.2, 5, layers=2)
    assert (d.weight_drop, d.variational_dropout, d.dropout_seed, d.layers) == (0.0, 0, 5, 2)
    d = Dk.decoder_dims(2, 3, 9, 6, 16, 8, 12, 20, 40, 11, True, 0, weight_drop=0.5, variational_dropout=True)
    assert (d.weight_drop, d.variational_dropout) == (0.5, 1)
    with pytest.raises(ValueError, match="weight_drop"):
        Dk.decoder_dims(2, 3, 9, 6, 16, 8, 12, 20, 40, 11, True, 0, weight_drop=1.0)


def test_header_declares_the_fields_in_the_same_order():
    text = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    body = text[text.index("typedef struct sat_decoder_dims {"):text.index("} sat_decoder_dims;")]
    assert body.index("uint64_t dropout_seed;") < body.index("float weight_drop;") < body.index("int32_t variational_dropout;")
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in text, name


def test_host_mask_is_dropout_scale_reference_on_stream_3():
    from sat_amd import decoder as Dk
    seed, n, p = 123456789, 20, 0.5
    s = Dk.weight_drop_scale_reference(seed, 3, n, p)
    assert s.shape == (3, 4 * n, n) and s.dtype == np.float32
    l, r, c = np.meshgrid(np.arange(3), np.arange(4 * n), np.arange(n), indexing="ij")
    assert np.array_equal(s, Dk.dropout_scale_reference(seed, 3, (l * 4 * n + r) * n + c, p))
    assert set(np.unique(s).tolist()) == {0.0, 2.0}
    for layer in range(3):                                     # a layer of the tall mask = that slice computed alone with its offset
        alone = Dk.weight_drop_scale_reference(seed, 1, n, p, layer0=layer)
        assert np.array_equal(alone[0], s[layer])
        off = layer * 4 * n * n
        assert np.array_equal(alone.ravel(), Dk.dropout_scale_reference(seed, 3, np.arange(off, off + 4 * n * n), p))
    # stream 3 is its own stream, and the seed matters
    assert not np.array_equal(s[0].ravel(), Dk.dropout_scale_reference(seed, 2, np.arange(4 * n * n), p))
    assert not np.array_equal(s, Dk.weight_drop_scale_reference(seed + 1, 3, n, p))
    kept = [float((s[layer] > 0).mean()) for layer in range(3)]
    assert all(abs(k - 0.5) < 0.05 for k in kept), kept
    assert bool((s > 0).any(axis=2).all())                     # no all-dropped row for this seed
    # any (layers, rows, cols) block, as the stand-alone entry points take it
    s2 = Dk.weight_drop_scale_reference(seed, 1, 5, 0.1, rows=20)
    assert s2.shape == (1, 20, 5) and np.array_equal(s2.ravel(), Dk.dropout_scale_reference(seed, 3, np.arange(100), 0.1))
    assert set(np.unique(s2).tolist()) <= {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)))}


def test_symbols_are_exported_and_bound_and_refuse_bad_arguments():
    from sat_amd import _lib as L
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and getattr(lib, name) is not None
    one = C.c_float(1.0)
    ptr = C.cast(C.pointer(one), C.c_void_p)
    bad = [dict(layers=0), dict(layers=L.MAX_LSTM_LAYERS + 1), dict(rows=0), dict(cols=-1), dict(p=1.0), dict(p=-0.5), dict(p=float("nan"))]
    for over in bad:                                           # refused before anything is launched: the pointers are host memory
        a = dict(layers=1, rows=1, cols=1, p=0.5)
        a.update(over)
        assert lib.sat_weight_drop(ptr, ptr, None, a["layers"], a["rows"], a["cols"], a["p"], 1, None) == SAT_EINVAL, over
        assert lib.sat_weight_drop_grad(ptr, a["layers"], a["rows"], a["cols"], a["p"], 1, None) == SAT_EINVAL, over
        assert lib.sat_last_error().decode()
    assert lib.sat_weight_drop(None, ptr, None, 1, 1, 1, 0.5, 1, None) == SAT_EINVAL
    assert lib.sat_weight_drop_grad(None, 1, 1, 1, 0.5, 1, None) == SAT_EINVAL
    d = L.DecoderDims(B=1, R=1, T=2, L=1, D=1, A=1, m=1, n=1, V=1, P=0, layers=1, weight_drop=1.0)
    assert lib.sat_decoder_workspace_bytes(C.byref(d)) == 0 and "weight_drop" in lib.sat_last_error().decode()
    d.weight_drop = -0.25
    assert lib.sat_decoder_workspace_bytes(C.byref(d)) == 0 and "weight_drop" in lib.sat_last_error().decode()
    assert lib.sat_decoder_pack_weights(C.byref(d), None, None, None, None, None) == SAT_EINVAL


def test_workspace_grows_only_for_stacked_layers_under_weight_drop():
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()

    def ws(layers, **kw):
        return lib.sat_decoder_workspace_bytes(C.byref(Dk.decoder_dims(2, 3, 9, 6, 16, 8, 12, 20, 40, 11, True, 0, layers=layers, **kw)))

    for layers in (1, 2, 3):
        base = ws(layers)
        assert base > 0 and ws(layers, variational_dropout=True) == base and ws(layers, weight_drop=0.0, dropout_seed=7) == base
        copies = (layers - 1) * 4 * 20 * 20 * 4                # fp32 copies of the stacked layers' W_hh, 256-byte granules
        assert ws(layers, weight_drop=0.5) == base + (copies + 255) // 256 * 256


def test_graphed_step_reports_dropout_for_weight_drop():
    from types import SimpleNamespace
    from sat_amd import graph as G
    step = G.GraphedTrainStep.__new__(G.GraphedTrainStep)
    step.enabled, step.opt = True, SimpleNamespace(step_device=None)
    img = SimpleNamespace(is_cuda=True)
    for hp, training, why in ((dict(weight_drop=0.5), True, "dropout"), (dict(weight_drop=0.5), False, None), (dict(weight_drop=0.0), True, None),
                              (dict(), True, None)):
        step.model = SimpleNamespace(hp=SimpleNamespace(dropout=0.0, embedding_dropout=0.0, **hp), training=training)
        assert step._why_eager(img) == why, (hp, training)
