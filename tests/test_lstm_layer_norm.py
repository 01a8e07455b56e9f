"""CPU: the layer-normalised LSTM cell ("Layer-normalised LSTM").  The hyper-parameter is checked at construction and off
by default; off, the state dict is the reference's; on, a sub-module ``lstm_ln`` holds gains (ones) and shifts (zeros) of every
layer; ``sat_decoder_params`` carries their pointers in its last four fields and a mixture of NULL and non-NULL is refused through
the C ABI before anything is launched; the decoder parameter list keeps its meaning; and the float64 reference step is the
``F.layer_norm`` composition and differentiable."""
import ctypes as C
import os

import pytest
import torch

import lstm_layer_norm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sat_decoder_workspace_bytes_ln", "sat_lstm_ln_slots", "sat_lstm_ln_cell_fwd", "sat_lstm_ln_cell_bwd", "sat_lstm_ln_param_grads",
               "sat_lstm_cell_pointwise_fwd", "sat_lstm_cell_pointwise_bwd")
SAT_EINVAL = 1                                                 # csrc/common.h


def small_hparams(**over):
    from oracle import sat_oracle as O
    return O.default_hparams(**dict(dict(vocab_size=40, encoder_dim=16, embed_dim=12, attention_dim=8, decoder_dim=20), **over))


@pytest.mark.parametrize("bad", ["yes", 0.5, 2, None, -1])
def test_lstm_layer_norm_other_than_a_flag_is_refused(bad):
    from sat_amd import model as M
    with pytest.raises(ValueError, match="lstm_layer_norm"):
        M.SATDecoder(small_hparams(lstm_layer_norm=bad))
    over = dict(vars(small_hparams(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=2)), lstm_layer_norm=bad)
    with pytest.raises(ValueError, match="lstm_layer_norm"):
        M.SAT(**over)


def test_off_by_default_and_the_state_dict_is_the_references():
    from sat_amd import model as M
    args = small_hparams(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=2, decoder_layers=2)
    assert not hasattr(args, "lstm_layer_norm")
    sat = M.SAT(**vars(args))
    assert sat.hp.lstm_layer_norm is False and not sat.lstm_layer_norm_on() and not hasattr(sat, "lstm_ln") and sat.ln_param_list() == []
    off = M.SAT(**dict(vars(args), lstm_layer_norm=False))
    assert list(off.state_dict()) == list(sat.state_dict()) and not any(k.startswith("lstm_ln") for k in sat.state_dict())
    dec = M.SATDecoder(small_hparams())                       # a namespace without the key
    assert not dec.lstm_layer_norm_on() and not any(k.startswith("lstm_ln") for k in dec.state_dict())
    assert dec._params_struct()[0].ln_gate_w[0] is None


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_on_the_parameters_exist_with_their_shapes_and_initial_values(layers):
    from sat_amd import _lib as L, model as M
    n = 20
    plain = M.SATDecoder(small_hparams(decoder_layers=layers))
    dec = M.SATDecoder(small_hparams(decoder_layers=layers, lstm_layer_norm=True))
    sd = dec.state_dict()
    assert [k for k in sd if k.startswith("lstm_ln.")] == R.ln_keys(layers)
    for k in R.ln_keys(layers):
        assert tuple(sd[k].shape) == ((4 * n,) if ".gates_" in k else (n,)) and sd[k].dtype == torch.float32
        assert bool((sd[k] == (1.0 if k.endswith("weight") else 0.0)).all()), k
    # lstm.* keys and shapes never change, and nothing else appears
    assert {k: tuple(v.shape) for k, v in sd.items() if not k.startswith("lstm_ln.")} == {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    # the group travels next to the parameter list in the order of _lib.ln_param_names
    group = dec.ln_param_list()
    assert len(group) == 4 * layers and len(dec.param_list()) == 18 + 4 * (layers - 1)
    for name, p in zip(L.ln_param_names(layers), group):
        assert p is dict(dec.named_parameters())[L.ln_param_key(name)]
    s, keep = dec._params_struct()
    for l in range(layers):
        for f, k in zip(L.LN_FIELDS, ("gates_l%d.weight", "gates_l%d.bias", "cell_l%d.weight", "cell_l%d.bias")):
            assert getattr(s, f)[l] == sd["lstm_ln." + k % l].data_ptr()
    for l in range(layers, L.MAX_LSTM_LAYERS):
        assert all(getattr(s, f)[l] is None for f in L.LN_FIELDS)
    assert set(L.ln_param_names(layers)) <= set(keep)


def test_loading_a_plain_checkpoint_leaves_the_norm_at_its_initial_values():
    from sat_amd import model as M
    plain = M.SATDecoder(small_hparams(decoder_layers=2))
    dec = M.SATDecoder(small_hparams(decoder_layers=2, lstm_layer_norm=True))
    dec.load_decoder_state(plain.state_dict())
    sd = dec.state_dict()
    for k, v in plain.state_dict().items():
        assert torch.equal(sd[k], v)
    for k in R.ln_keys(2):
        assert bool((sd[k] == (1.0 if k.endswith("weight") else 0.0)).all())
    fresh = M.SATDecoder(small_hparams(decoder_layers=2, lstm_layer_norm=True))
    with torch.no_grad():
        for p in dec.ln_param_list():
            p.uniform_(-1, 1)
    fresh.load_state_dict(dec.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(fresh.ln_param_list(), dec.ln_param_list()))


def test_optimizer_puts_the_new_parameters_into_the_decoders_no_decay_group():
    from sat_amd import model as M
    kw = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=2, weight_decay=0.1, decoder_lr=1e-3, embedding_lr=1e-2, encoder_lr=1e-4,
              opt="sgd", adam_b1=0.9, adam_b2=0.999, momentum=0.9, nesterov=False, scheduler=None, fused_optimizer=False, decoder_layers=2,
              lstm_layer_norm=True)
    sat = M.SAT(**vars(small_hparams(**kw)))
    opt = sat.configure_optimizers()
    no_decay, decay = opt.param_groups[0], opt.param_groups[1]
    assert no_decay["weight_decay"] == 0.0 and decay["weight_decay"] == 0.1
    ids = {id(p) for p in no_decay["params"]}
    assert all(id(p) in ids for p in sat.ln_param_list()) and not any(id(p) in {id(q) for q in decay["params"]} for p in sat.ln_param_list())


def test_params_struct_ends_with_the_four_fields_in_the_headers_order():
    from sat_amd import _lib as L
    names = [f[0] for f in L.DecoderParams._fields_]
    assert names[-4:] == ["ln_gate_w", "ln_gate_b", "ln_cell_w", "ln_cell_b"] == list(L.LN_FIELDS)
    assert names[:-4] == list(L.PARAM_FIELDS) + list(L.UP_FIELDS)
    ptr = C.sizeof(C.c_void_p)
    assert L.DecoderParams.ln_gate_w.offset == (len(L.PARAM_FIELDS) + 4 * (L.MAX_LSTM_LAYERS - 1)) * ptr
    for a, b in zip(L.LN_FIELDS, L.LN_FIELDS[1:]):
        assert getattr(L.DecoderParams, b).offset == getattr(L.DecoderParams, a).offset + L.MAX_LSTM_LAYERS * ptr
    assert C.sizeof(L.DecoderParams) == L.DecoderParams.ln_cell_b.offset + L.MAX_LSTM_LAYERS * ptr
    s = L.DecoderParams(embedding=1)                          # a construction from before the fields existed: zero-filled = the plain cell
    assert all(getattr(s, f)[l] is None for f in L.LN_FIELDS for l in range(L.MAX_LSTM_LAYERS))
    text = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    body = text[text.index("typedef struct sat_decoder_params {"):text.index("} sat_decoder_params;")]
    order = [body.index("float* %s[SAT_MAX_LSTM_LAYERS]" % f) for f in L.LN_FIELDS]
    assert body.index("up_b_hh[SAT_MAX_LSTM_LAYERS - 1]") < order[0] and order == sorted(order)
    # sat_decoder_dims did not change
    assert [f[0] for f in L.DecoderDims._fields_][-3:] == ["dropout_seed", "weight_drop", "variational_dropout"]


def test_abi_version_stays_and_the_new_symbols_are_declared_exported_and_bound():
    from sat_amd import _lib as L
    lib = L.lib()
    text = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    assert "#define SAT_HIP_ABI_VERSION 23" in text and lib.sat_abi_version() == 23
    for name in NEW_SYMBOLS:
        assert " %s(" % name in text and name in L.SYMBOLS and getattr(lib, name) is not None, name
    assert [lib.sat_lstm_ln_slots(r) for r in (1, 7, 1024, 1025, 100000)] == [1, 7, 1024, 1024, 1024]


def test_parameter_list_keeps_its_meaning():
    from sat_amd import _lib as L, decoder as Dk
    assert [Dk.layers_of(k) for k in (18, 22, 26, 30)] == [1, 2, 3, 4]
    for bad in (17, 19, 20, 21, 23):
        with pytest.raises(ValueError):
            Dk.layers_of(bad)
    assert L.param_names(1) == list(L.PARAM_FIELDS) and len(L.param_names(2)) == 22 and L.param_names(2)[18:] == ["w_ih_l1", "w_hh_l1", "b_ih_l1", "b_hh_l1"]
    assert not any(k.startswith("ln_") for layers in (1, 2, 3, 4) for k in L.param_names(layers))
    assert L.ln_param_names(2) == ["ln_gate_w_l0", "ln_gate_b_l0", "ln_cell_w_l0", "ln_cell_b_l0", "ln_gate_w_l1", "ln_gate_b_l1", "ln_cell_w_l1", "ln_cell_b_l1"]
    assert [L.ln_param_key(k) for k in L.ln_param_names(1)] == R.ln_keys(1)
    # the trailing group is split off by its explicit count: 22 tensors are two layers, or one layer and its norm
    t = [torch.zeros(1) for _ in range(22)]
    assert [len(x) for x in Dk.split_ln(t, 0)] == [22, 0] and [len(x) for x in Dk.split_ln(t, 4)] == [18, 4]
    for bad in (3, 8, -4):
        with pytest.raises(ValueError):
            Dk.split_ln(t, bad)
    # _params_struct without the group is what it was
    tens = {k: torch.zeros(2) for k in L.param_names(2)}
    s = Dk._params_struct(tens, 2)
    assert s.embedding == tens["embedding"].data_ptr() and s.up_w_ih[0] == tens["w_ih_l1"].data_ptr() and s.ln_gate_w[0] is None


def test_a_mixture_of_null_and_set_norm_tensors_is_refused_before_any_launch():
    from sat_amd import _lib as L
    lib = L.lib()
    one = C.c_float(1.0)
    some = C.cast(C.pointer(one), C.c_void_p).value
    d = L.DecoderDims(B=1, R=1, T=2, L=1, D=1, A=1, m=1, n=1, V=1, P=0, deep_output=0, layers=2)
    offs = (C.c_int32 * 2)(0, 0); teach = (C.c_int32 * 1)(1)
    b = L.DecoderBatch(ann=some, caps=some, lengths=some, prow=some, src_row=some, step_offsets_host=C.cast(offs, C.c_void_p).value,
                       teacher_host=C.cast(teach, C.c_void_p).value)

    def params(ln):
        w = L.DecoderParams(**{k: some for k in L.PARAM_FIELDS})
        for f in L.UP_FIELDS:
            getattr(w, f)[0] = some
        for f, l in ln:
            getattr(w, f)[l] = some
        return w

    full = [(f, l) for l in range(2) for f in L.LN_FIELDS]
    for ln in ([("ln_gate_w", 0)], full[:-1], full[:4], [("ln_cell_b", 1)], full[1:]):
        w = params(ln)
        assert lib.sat_decoder_train_fwd(C.byref(d), C.byref(w), C.byref(b), None, None, None, 0, None) == SAT_EINVAL, ln
        msg = lib.sat_last_error().decode()
        assert "layer-norm" in msg and "all or none" in msg, msg
        assert lib.sat_decoder_infer_begin(C.byref(d), C.byref(w), None, 1, 1, None, None, None, 0, None) == SAT_EINVAL and "layer-norm" in lib.sat_last_error().decode()
    # all or none pass this check (the next one, the NULL outputs, answers)
    for ln in ([], full):
        assert lib.sat_decoder_train_fwd(C.byref(d), C.byref(params(ln)), C.byref(b), None, None, None, 0, None) == SAT_EINVAL
        assert "layer-norm" not in lib.sat_last_error().decode()
    # the stand-alone launches refuse NULL and bad shapes
    p = C.c_void_p(some)
    assert lib.sat_lstm_ln_cell_fwd(None, 4, None, p, p, p, p, None, None, p, p, p, p, None, None, 1, 1, None) == SAT_EINVAL
    assert lib.sat_lstm_ln_cell_fwd(p, 3, None, p, p, p, p, None, None, p, p, p, p, None, None, 1, 1, None) == SAT_EINVAL and "g_ld" in lib.sat_last_error().decode()
    assert lib.sat_lstm_ln_cell_fwd(p, 4, None, p, p, p, p, None, None, p, p, p, p, p, None, 1, 1, None) == SAT_EINVAL and "together" in lib.sat_last_error().decode()
    assert lib.sat_lstm_ln_cell_bwd(p, 4, p, None, p, None, p, p, p, 4, None, None, p, p, p, None, 1, 1, None) == SAT_EINVAL
    assert lib.sat_lstm_ln_cell_bwd(p, 4, p, p, p, None, p, p, p, 3, None, None, p, p, p, None, 1, 1, None) == SAT_EINVAL and "dg_ld" in lib.sat_last_error().decode()
    assert lib.sat_lstm_ln_param_grads(p, 0, 1, p, p, p, p, p, None) == SAT_EINVAL
    assert lib.sat_lstm_ln_param_grads(p, 1025, 1, p, p, p, p, p, None) == SAT_EINVAL


def test_workspace_grows_only_with_the_norm():
    from sat_amd import _lib as L, decoder as Dk
    lib = L.lib()
    one = C.c_float(1.0)
    some = C.cast(C.pointer(one), C.c_void_p).value
    Bn, Rn, Tn, n = 2, 3, 9, 20
    for layers in (1, 2, 3):
        d = Dk.decoder_dims(Bn, Rn, Tn, 6, 16, 8, 12, n, 40, 11, True, 0, layers=layers)
        base = lib.sat_decoder_workspace_bytes(C.byref(d))
        w = L.DecoderParams()
        assert base > 0 and lib.sat_decoder_workspace_bytes_ln(C.byref(d), None) == base and lib.sat_decoder_workspace_bytes_ln(C.byref(d), C.byref(w)) == base
        for f in L.LN_FIELDS:
            for l in range(layers):
                getattr(w, f)[l] = some
        N, T1 = Bn * Rn, Tn - 1
        up = lambda x: (x + 255) // 256 * 256
        extra = up(layers * T1 * N * 5 * n * 4) + up(layers * T1 * N * 5 * 4) + up(layers * lib.sat_lstm_ln_slots(N) * 10 * n * 4)
        assert lib.sat_decoder_workspace_bytes_ln(C.byref(d), C.byref(w)) == base + extra


def test_graph_key_carries_the_flag():
    import inspect
    from sat_amd import graph as G
    assert "lstm_layer_norm_on()" in inspect.getsource(G.GraphedTrainStep)


# ------------------------------------------------------------------ the reference step
def ref_inputs(layers, n=5, inp=7, N=3, seed=3, dtype=torch.float64):
    from oracle import prng
    hp = small_hparams(decoder_dim=n, embed_dim=3, encoder_dim=inp - 3, decoder_layers=layers)
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in prng.decoder_state(hp, seed).items() if k.startswith("lstm.")}
    sd.update({k: v.to(dtype) for k, v in R.ln_state(n, layers, seed + 50).items()})
    x = torch.from_numpy(prng.uniform((1, N, inp), seed + 1)).to(dtype)
    h = torch.from_numpy(prng.uniform((layers, N, n), seed + 2)).to(dtype)
    c = torch.from_numpy(prng.uniform((layers, N, n), seed + 3)).to(dtype)
    return sd, x, h, c


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_reference_step_is_the_layer_norm_composition(layers):
    sd, x, h, c = ref_inputs(layers)
    hn, cn = R.ln_lstm_step(sd, x, h, c, layers)
    hl, cl = R.ln_lstm_step_layer_norm(sd, x, h, c, layers)
    assert hn.dtype == torch.float64 and hn.shape == h.shape and cn.shape == c.shape
    assert float((hn - hl).abs().max()) < 1e-12 and float((cn - cl).abs().max()) < 1e-12
    # gains of one and shifts of zero are not the plain cell: the norm itself acts
    from oracle import sat_oracle as O
    hp_, cp_ = O.lstm_step_math(sd, x, h, c, layers)
    assert float((hn - hp_).abs().max()) > 1e-3
    # every gain and shift matters
    for k in R.ln_keys(layers):
        sd2 = dict(sd); sd2[k] = sd[k] + 0.25
        h2, _ = R.ln_lstm_step(sd2, x, h, c, layers)
        assert float((h2 - hn).abs().max()) > 1e-6, k
    # float32 in, float32 out
    sd32 = {k: v.float() for k, v in sd.items()}
    h32, _ = R.ln_lstm_step(sd32, x.float(), h.float(), c.float(), layers)
    assert h32.dtype == torch.float32 and float((h32.double() - hn).abs().max()) < 1e-5


@pytest.mark.parametrize("layers", [1, 2])
def test_reference_step_passes_gradcheck(layers):
    sd, x, h, c = ref_inputs(layers, n=4, inp=5, N=2)
    keys = sorted(sd)
    leaves = [sd[k].clone().requires_grad_() for k in keys] + [x.clone().requires_grad_(), h.clone().requires_grad_(), c.clone().requires_grad_()]

    def fn(*args):
        return R.ln_lstm_step(dict(zip(keys, args[:len(keys)])), args[-3], args[-2], args[-1], layers)

    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_cell_parts_are_the_saved_quantities():
    sd, x, h, c = ref_inputs(1, n=6)
    n = 6
    a = torch.nn.functional.linear(x[0], sd["lstm.weight_ih_l0"], sd["lstm.bias_ih_l0"]) + torch.nn.functional.linear(h[0], sd["lstm.weight_hh_l0"], sd["lstm.bias_hh_l0"])
    out = R.ln_cell(a, c[0], *[sd["lstm_ln.%s_l0.%s" % mp] for mp in (("gates", "weight"), ("gates", "bias"), ("cell", "weight"), ("cell", "bias"))])
    hn, cn = R.ln_lstm_step(sd, x, h, c, 1)
    assert torch.equal(out["h"], hn[0]) and torch.equal(out["c"], cn[0])
    assert out["xhat"].shape == (3, 5 * n) and out["rstd"].shape == (3, 5) and out["gates"].shape == (3, 4 * n)
    for k in range(5):
        xh = out["xhat"][:, k * n:(k + 1) * n]
        assert float(xh.mean(dim=1).abs().max()) < 1e-12 and float(((xh ** 2).mean(dim=1) + R.EPS * out["rstd"][:, k] ** 2 - 1).abs().max()) < 1e-12
