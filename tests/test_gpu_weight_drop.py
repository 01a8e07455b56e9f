"""GPU: weight-drop and variational dropout in the decoder train step ("Weight-drop and variational dropout").

Every mask is the stateless counter hash of the kernels, so the host rebuilds it exactly (``decoder.weight_drop_scale_reference`` /
``dropout_scale_reference``) and the tests are exact wherever both sides compute the same fp32 product of the same operands:
  1. the stand-alone kernels and the packing launch in NaN frames, bit for bit;
  2. / 3. a decoder with ``weight_drop`` against a decoder whose ``weight_hh_l*`` were multiplied by the host mask beforehand: logits,
     alphas and every gradient bit for bit (the weight gradient of the hidden-to-hidden matrices = mask * the other run's);
  4. against the CPU oracle with ``weight_hh_l* = leaf * mask`` at the tolerances of test_gpu_decoder.py (1e-4 / 2e-4);
  5. variational dropout against the oracle fed with locked masks;
  6. eval mode, seeds, and the graphed step's fallback.
Sizes: those of test_dropout_matches_oracle_with_the_same_masks with A = 7, D = 24, so that W_hh starts at element (A + D) n = 620 of
Wcat, inside a 256-thread block of the packing launch."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
SEED = 123456789
B, R, T, V, HH, WW = 4, 3, 9, 40, 2, 3
DRAWS = [0.9, 0.1, 0.8, 0.2, 0.7, 0.3]
SMALL = dict(A=7, D=24, m=12, n=20)
ALIGNED = dict(A=8, D=64, m=12, n=64)            # bf16 mode keeps bf16 operand copies (Wcat_b) only at n % 64 == D % 64 == 0


def close(a, b, tol=TOL, what=""):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    assert err <= tol * scale, "%s: max|d|=%.3e (scale %.3g, tol %.1e)" % (what, err, scale, tol)
    return err


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    itype = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(itype), b.view(itype))


@pytest.fixture(scope="module")
def M():
    import sat_amd  # noqa: F401
    from sat_amd import model
    return model


def make_hp(layers=1, shape="small", **over):
    from oracle import sat_oracle as O
    s = SMALL if shape == "small" else ALIGNED
    return O.default_hparams(vocab_size=V, encoder_dim=s["D"], embed_dim=s["m"], attention_dim=s["A"], decoder_dim=s["n"], decoder_layers=layers, **over)


@functools.lru_cache(maxsize=None)
def inputs(layers, shape="small"):
    """(state dict, annotations (B, D, h, w), captions, ragged lengths): read-only, shared by every test"""
    from oracle import prng
    hp = make_hp(layers, shape)
    sd = {k: torch.from_numpy(v) for k, v in prng.decoder_state(hp, 91 + layers).items()}
    ann = torch.from_numpy(prng.uniform((B, hp.encoder_dim, HH, WW), 911))
    caps, lengths = prng.captions(B, R, T, V, 912)
    lengths = torch.from_numpy(lengths)
    assert len(set(lengths.reshape(-1).tolist())) > 2           # ragged: the packed-row -> caption-row map is not the identity
    return sd, ann, torch.from_numpy(caps), lengths


def wd_mask(layers, n, p=0.5, seed=SEED):
    from sat_amd import decoder as Dk
    return torch.from_numpy(Dk.weight_drop_scale_reference(seed, layers, n, p))


def premask(sd, mask):
    out = dict(sd)
    for l in range(mask.shape[0]):
        out["lstm.weight_hh_l%d" % l] = sd["lstm.weight_hh_l%d" % l] * mask[l]
    return out


def decode(M, hp, sd, layers, shape="small", eps=1.0, precision="fp32", train=True, seed=SEED, backward=True, reg=False):
    """one train_decode (+ backward) of a fresh decoder; everything comes back on the host"""
    _, ann, caps, lengths = inputs(layers, shape)
    dec = M.SATDecoder(hp).cuda()
    dec.load_decoder_state(sd)
    dec.train(train)
    dec.sat_precision = precision
    ann_bld = ann.permute(0, 2, 3, 1).reshape(B, HH * WW, hp.encoder_dim).contiguous().cuda().requires_grad_()
    it = iter(DRAWS)
    res = dec.train_decode(ann_bld, caps.cuda(), lengths, eps, draw=lambda: next(it), dropout_seed=seed)
    out = dict(logits=res["logits_packed"].detach().cpu(), alphas=res["alphas"].detach().cpu(), plan=res["plan"])
    if backward:
        loss = res["ce"] + res["ds"]
        if reg:
            loss = dec.add_reg_terms(loss, res["reg"])
            out.update(ar=res["ar"].cpu(), tar=res["tar"].cpu())
        loss.backward()
        torch.cuda.synchronize()
        out.update(loss=loss.detach().cpu(), d_ann=ann_bld.grad.cpu(), grads={k: p.grad.cpu() for k, p in dec.named_parameters()})
    return out


# ---------------------------------------------------------------------------------------------- 1. the kernels alone
def framed(numel, dtype=torch.float32, guard=64):
    buf = torch.full((numel + 2 * guard,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[guard:guard + numel]


def guards_intact(buf, numel, guard=64):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + numel:]).all())


@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("shape", [(1, 4, 1), (1, 20, 5), (3, 80, 20), (1, 256, 64)])
def test_weight_drop_kernels_in_nan_frames(shape, p):
    from oracle import prng
    from sat_amd import decoder as Dk
    layers, rows, cols = shape
    numel = layers * rows * cols
    w = torch.from_numpy(prng.uniform(shape, 5))
    mask = torch.from_numpy(Dk.weight_drop_scale_reference(SEED, layers, cols, p, rows=rows))
    assert mask.shape == w.shape
    wbuf, wv = framed(numel); obuf, ov = framed(numel); bbuf, bv = framed(numel, torch.bfloat16); gbuf, gv = framed(numel)
    wv.copy_(w.reshape(-1)); gv.copy_(w.reshape(-1))
    Dk.weight_drop(wv.view(shape), p, SEED, out=ov.view(shape), out_bf16=bv.view(shape))
    Dk.weight_drop_grad_(gv.view(shape), p, SEED)
    torch.cuda.synchronize()
    want = w * mask                                             # one fp32 product per element, as on the device
    assert bits_equal(ov.view(shape), want), "out_f32"
    assert bits_equal(bv.view(shape), want.to(torch.bfloat16)), "out_bf16"
    assert bits_equal(gv.view(shape), want), "gradient masked in place"
    assert bits_equal(wv.view(shape), w), "the input is read only"
    for buf in (wbuf, obuf, bbuf, gbuf):
        assert guards_intact(buf, numel)
    # without the bf16 output, and in place
    o2, none = Dk.weight_drop(wv.view(shape), p, SEED)
    assert none is None and bits_equal(o2, want)
    Dk.weight_drop(wv.view(shape), p, SEED, out=wv.view(shape))
    assert bits_equal(wv.view(shape), want) and guards_intact(wbuf, numel)


def test_weight_drop_keeps_the_expected_share():
    from sat_amd import decoder as Dk
    shape, p = (3, 80, 20), 0.5
    out, _ = Dk.weight_drop(torch.ones(shape, device="cuda"), p, SEED)
    mask = torch.from_numpy(Dk.weight_drop_scale_reference(SEED, 3, 20, p))
    assert bits_equal(out, mask)
    kept = (out.cpu() > 0).float().mean(dim=(1, 2)).tolist()
    print("kept share per layer:", kept)                         # host replica: 0.5106 / 0.5006 / 0.5113
    assert all(abs(k - (1 - p)) <= 0.05 for k in kept), kept
    assert bool((out.cpu() > 0).any(dim=2).all())                # no all-dropped row for this seed


@pytest.mark.parametrize("with_bf16", [False, True])
@pytest.mark.parametrize("p", [0.5, 0.1, 0.0])
def test_packing_launch_masks_the_recurrent_rows_only(p, with_bf16):
    """Wcat = [W_d ; W_beta ; W_hh * s] with the hash index relative to W_hh; bcat is untouched by the mask"""
    import ctypes as C
    from sat_amd import _lib as L, decoder as Dk
    A, D, m, n = (SMALL[k] for k in ("A", "D", "m", "n"))
    sd = inputs(1)[0]
    names = {"att_dec": "attention.decoder_att.weight", "beta_w": "beta.0.weight", "w_hh": "lstm.weight_hh_l0", "beta_b": "beta.0.bias",
             "b_ih": "lstm.bias_ih_l0", "b_hh": "lstm.bias_hh_l0"}
    tens = {k: sd[v].cuda().contiguous() for k, v in names.items()}
    HCW = A + D + 4 * n
    assert (A + D) * n == 620 and 620 % 256 != 0
    wbuf, wv = framed(HCW * n); bbuf, bv = framed(HCW * n, torch.bfloat16); cbuf, cv = framed(HCW)
    dims = Dk.decoder_dims(B, R, T, HH * WW, D, A, m, n, V, 0, True, 0, weight_drop=p, dropout_seed=SEED)
    L.check(L.lib().sat_decoder_pack_weights(C.byref(dims), C.byref(Dk._params_struct(tens)), L.ptr(wv), L.ptr(bv) if with_bf16 else None, L.ptr(cv),
                                             L.stream_ptr()), "sat_decoder_pack_weights")
    torch.cuda.synchronize()
    w_hh = sd["lstm.weight_hh_l0"] * wd_mask(1, n, p)[0] if p > 0 else sd["lstm.weight_hh_l0"]
    want = torch.cat([sd[names["att_dec"]], sd[names["beta_w"]], w_hh]).reshape(-1)
    assert bits_equal(wv, want)
    if with_bf16:
        assert bits_equal(bv, want.to(torch.bfloat16))
    else:
        assert bool(torch.isnan(bv.float()).all())
    assert bits_equal(cv, torch.cat([torch.zeros(A), sd[names["beta_b"]], sd[names["b_ih"]] + sd[names["b_hh"]]]))
    assert guards_intact(wbuf, HCW * n) and guards_intact(bbuf, HCW * n) and guards_intact(cbuf, HCW)


# ---------------------------------------------------------------------------------------------- 2. / 3. against pre-masked weights
PAIRS = [(1, "fp32", 1.0, "small"), (2, "fp32", 1.0, "small"), (3, "fp32", 1.0, "small"), (1, "bf16", 1.0, "small"),
         (1, "fp32", 0.5, "small"), (2, "fp32", 0.5, "small"), (3, "fp32", 0.5, "small"), (1, "bf16", 0.5, "small"),
         (1, "bf16", 1.0, "aligned"), (1, "bf16", 0.5, "aligned")]
_pairs = {}


def pair(M, layers, precision, eps, shape):
    """(run with weight_drop = 0.5, run of the pre-masked weights with weight_drop = 0, host mask): computed once per case"""
    key = (layers, precision, eps, shape)
    if key not in _pairs:
        sd = inputs(layers, shape)[0]
        mask = wd_mask(layers, make_hp(layers, shape).decoder_dim)
        got = decode(M, make_hp(layers, shape, weight_drop=0.5), sd, layers, shape, eps, precision)
        ref = decode(M, make_hp(layers, shape), premask(sd, mask), layers, shape, eps, precision)
        _pairs[key] = (got, ref, mask)
    return _pairs[key]


@pytest.mark.parametrize("layers,precision,eps,shape", PAIRS)
def test_forward_equals_the_premasked_weights_bit_for_bit(M, layers, precision, eps, shape):
    got, ref, mask = pair(M, layers, precision, eps, shape)
    assert torch.equal(got["logits"], ref["logits"]) and torch.equal(got["alphas"], ref["alphas"])
    assert torch.isfinite(got["logits"]).all()
    # ... and the mask matters: the plain weights give other logits
    plain = decode(M, make_hp(layers, shape), inputs(layers, shape)[0], layers, shape, eps, precision, backward=False)
    assert not torch.equal(plain["logits"], got["logits"])


@pytest.mark.parametrize("layers,precision,eps,shape", PAIRS)
def test_gradients_equal_the_premasked_run_and_the_mask_bit_for_bit(M, layers, precision, eps, shape):
    got, ref, mask = pair(M, layers, precision, eps, shape)
    assert torch.equal(got["loss"], ref["loss"]) and torch.equal(got["d_ann"], ref["d_ann"])
    hh = {"lstm.weight_hh_l%d" % l: l for l in range(layers)}
    assert set(hh) <= set(got["grads"])
    for k, g in got["grads"].items():
        if k not in hh:
            assert torch.equal(g, ref["grads"][k]), "gradient of %s" % k
            continue
        s = mask[hh[k]]
        assert bits_equal(g, s * ref["grads"][k]), "gradient of %s is not mask * the gradient w.r.t. the masked matrix" % k
        assert float(g[s == 0].abs().max()) == 0.0               # a dropped position has gradient exactly 0
        assert float(g[s > 0].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------- 4. against the oracle
def oracle_leaves(sd, mask):
    """(leaves, state dict for the oracle): the oracle sees weight_hh_l* = leaf * mask, the gradients land on the leaves"""
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    sdo = dict(leaves)
    for l in range(mask.shape[0]):
        sdo["lstm.weight_hh_l%d" % l] = leaves["lstm.weight_hh_l%d" % l] * mask[l]
    return leaves, sdo


def compare_with_oracle(got, loss_o, out_o, leaves, ann_o, what):
    close(got["logits"], out_o["logits_packed"], what="logits " + what)
    close(got["alphas"], out_o["alphas"], what="alphas " + what)
    close(got["loss"], loss_o, what="loss " + what)
    close(got["d_ann"].reshape(B, HH, WW, -1).permute(0, 3, 1, 2), ann_o.grad, 2e-4, "d_ann " + what)
    for k, g in got["grads"].items():
        close(g, leaves[k].grad, 2e-4, k + " " + what)


@pytest.mark.parametrize("layers", [1, 2])
def test_weight_drop_against_the_oracle(M, layers):
    from oracle import sat_oracle as O
    sd, ann, caps, lengths = inputs(layers)
    hp = make_hp(layers, weight_drop=0.5)
    got = decode(M, hp, sd, layers)
    leaves, sdo = oracle_leaves(sd, wd_mask(layers, hp.decoder_dim))
    ann_o = ann.clone().requires_grad_()
    loss_o, out_o = O.training_loss(sdo, hp, ann_o, caps, lengths, 1.0)
    loss_o.backward()
    compare_with_oracle(got, loss_o, out_o, leaves, ann_o, "under weight-drop")


def host_dropout_masks(plan, N, D, m, p, pe, locked):
    """the oracle's masks=: init (N, D), emb (T1, N, m), out (T1, N, m); ``locked``: one row per caption for all steps"""
    from sat_amd import decoder as Dk
    T1 = T - 1
    sc = lambda stream, count, rate: torch.from_numpy(Dk.dropout_scale_reference(SEED, stream, np.arange(count), rate))
    init = sc(0, N * D, p).reshape(N, D)
    prow = plan.prow.cpu()
    live = prow >= 0
    if locked:
        emb = sc(1, N * m, pe).reshape(1, N, m).repeat(T1, 1, 1)
        out = sc(2, N * m, p).reshape(1, N, m).repeat(T1, 1, 1) * live.unsqueeze(-1)
    else:
        emb = sc(1, T1 * N * m, pe).reshape(T1, N, m)
        packed = sc(2, plan.P * m, p).reshape(plan.P, m)
        out = torch.zeros(T1, N, m)
        out[live] = packed[prow[live].long()]
    return dict(init=init, emb=emb, out=out)


def test_weight_drop_with_the_dropouts_and_activation_regularisation_against_the_oracle(M):
    """everything of the recipe in one step: weight-drop, the three per-step dropouts, AR / TAR, two layers, scheduled sampling"""
    import activation_reg_ref as AR
    from oracle import sat_oracle as O
    layers, p, pe, ar_alpha, tar_beta = 2, 0.3, 0.2, 2.0, 1.0
    sd, ann, caps, lengths = inputs(layers)
    hp = make_hp(layers, weight_drop=0.5, dropout=p, embedding_dropout=pe, ar_alpha=ar_alpha, tar_beta=tar_beta)
    got = decode(M, hp, sd, layers, eps=0.5, reg=True)
    N, lens = B * R, lengths.reshape(-1)
    masks = host_dropout_masks(got["plan"], N, hp.encoder_dim, hp.embed_dim, p, pe, locked=False)
    leaves, sdo = oracle_leaves(sd, wd_mask(layers, hp.decoder_dim))
    ann_o = ann.clone().requires_grad_()
    hidden = []

    def lstm_fn(sd_, x, h, c, nl):                              # the oracle's step; keeps the top-layer state of the live rows
        hn, cn = O.lstm_step(sd_, x, h, c, nl)
        full = torch.zeros(N, hp.decoder_dim)
        full[lens > len(hidden)] = hn[-1]
        hidden.append(full)
        return hn, cn

    it = iter(DRAWS)
    out_o = O.decode_train(sdo, hp, ann_o, caps, lengths, 0.5, lambda: next(it), lstm_fn=lstm_fn, masks=masks)
    while len(hidden) < T - 1:
        hidden.append(torch.zeros(N, hp.decoder_dim))
    lp, _ = O.pack_time_major(out_o["logits"], out_o["lengths"])
    tp, _ = O.pack_time_major(out_o["targets"], out_o["lengths"])
    ar, tar, _, _ = AR.reg_terms(torch.stack(hidden).double(), lens)
    loss_o = O.label_smoothing_ce(lp, tp, hp.label_smoothing) + O.doubly_stochastic(out_o["alphas"], hp.att_gamma) + (ar_alpha * ar + tar_beta * tar).float()
    loss_o.backward()
    out_o["logits_packed"] = lp
    close(got["ar"], ar, what="ar"); close(got["tar"], tar, what="tar")
    compare_with_oracle(got, loss_o, out_o, leaves, ann_o, "under weight-drop, dropout and AR / TAR")


# ---------------------------------------------------------------------------------------------- 5. variational dropout
@pytest.mark.parametrize("eps", [1.0, 0.5])
def test_variational_dropout_against_the_oracle_with_locked_masks(M, eps):
    from oracle import sat_oracle as O
    layers, p, pe = 1, 0.3, 0.2
    sd, ann, caps, lengths = inputs(layers)
    hp = make_hp(layers, dropout=p, embedding_dropout=pe, variational_dropout=True)
    got = decode(M, hp, sd, layers, eps=eps)
    N = B * R
    masks = host_dropout_masks(got["plan"], N, hp.encoder_dim, hp.embed_dim, p, pe, locked=True)
    for t in range(1, T - 1):                                    # one mask row per caption for all of its time steps
        assert torch.equal(masks["emb"][t], masks["emb"][0])
        live = got["plan"].prow.cpu()[t] >= 0                    # every caption is live at step 0
        assert torch.equal(masks["out"][t][live], masks["out"][0][live])
    kept_emb, kept_out = float((masks["emb"][0] > 0).float().mean()), float((masks["out"][0] > 0).float().mean())
    print("kept: embedding %.4f, output %.4f" % (kept_emb, kept_out))         # host: 0.8125 and 0.646
    assert abs(kept_emb - (1 - pe)) <= 0.1 and abs(kept_out - (1 - p)) <= 0.1
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ann_o = ann.clone().requires_grad_()
    it = iter(DRAWS)
    loss_o, out_o = O.training_loss(leaves, hp, ann_o, caps, lengths, eps, draw=lambda: next(it), masks=masks)
    loss_o.backward()
    compare_with_oracle(got, loss_o, out_o, leaves, ann_o, "under variational dropout")
    # the per-step masks are other masks: the same run with variational_dropout=False does not match the locked ones ...
    per_step = decode(M, make_hp(layers, dropout=p, embedding_dropout=pe), sd, layers, eps=eps, backward=False)
    scale = max(1.0, float(out_o["logits_packed"].detach().abs().max()))
    assert float((per_step["logits"] - out_o["logits_packed"].detach()).abs().max()) > 100 * TOL * scale
    # ... and matches its own
    masks_t = host_dropout_masks(per_step["plan"], N, hp.encoder_dim, hp.embed_dim, p, pe, locked=False)
    it = iter(DRAWS)
    with torch.no_grad():
        _, out_t = O.training_loss(sd, hp, ann, caps, lengths, eps, draw=lambda: next(it), masks=masks_t)
    close(per_step["logits"], out_t["logits_packed"], what="per-step masks")


def test_variational_dropout_without_a_rate_does_nothing(M):
    sd = inputs(1)[0]
    on = decode(M, make_hp(1, variational_dropout=True), sd, 1)
    off = decode(M, make_hp(1), sd, 1)
    assert torch.equal(on["logits"], off["logits"]) and all(torch.equal(g, off["grads"][k]) for k, g in on["grads"].items())


# ---------------------------------------------------------------------------------------------- 6. modes
def test_eval_mode_is_the_identity_and_seeds_decide_the_masks(M):
    layers = 2
    sd = inputs(layers)[0]
    both = dict(weight_drop=0.5, variational_dropout=True, dropout=0.3, embedding_dropout=0.2)
    ev = decode(M, make_hp(layers, **both), sd, layers, train=False, backward=False)
    plain = decode(M, make_hp(layers), sd, layers, train=False, backward=False)
    assert torch.equal(ev["logits"], plain["logits"]) and torch.equal(ev["alphas"], plain["alphas"])
    a = decode(M, make_hp(layers, **both), sd, layers)
    b = decode(M, make_hp(layers, **both), sd, layers)
    assert torch.equal(a["logits"], b["logits"]) and all(torch.equal(g, b["grads"][k]) for k, g in a["grads"].items())
    c = decode(M, make_hp(layers, **both), sd, layers, seed=SEED + 1)
    assert not torch.equal(a["logits"], c["logits"])
    wd_only = decode(M, make_hp(layers, weight_drop=0.5), sd, layers, backward=False)
    wd_other = decode(M, make_hp(layers, weight_drop=0.5), sd, layers, seed=SEED + 1, backward=False)
    assert not torch.equal(wd_only["logits"], wd_other["logits"]) and not torch.equal(wd_only["logits"], plain["logits"])


def test_graphed_step_falls_back_to_the_eager_step_under_weight_drop():
    import sat_amd  # noqa: F401
    from oracle import prng, sat_oracle as O
    from sat_amd import model as Mo
    from sat_amd.graph import GraphedTrainStep
    kw = dict(encoder_arch="resnet18", encoder_dim=64, input_size=64, encoder_size=3, vocab_size=120, embed_dim=24, attention_dim=16,
              decoder_dim=40, deep_output=True, weight_decay=0.0, decoder_lr=1e-3, embedding_lr=1e-2, encoder_lr=1e-4, opt="adam",
              adam_b1=0.9, adam_b2=0.999, momentum=0.9, nesterov=False, scheduler=None, decoder_tf="always", encoder_finetune_after=1,
              lr_warmup_steps=4, weight_drop=0.5)
    hp = O.default_hparams(**kw)
    models = []
    for _ in range(2):                                           # one seed: the same parameters and the same stream of mask seeds
        torch.manual_seed(42)
        models.append(Mo.SAT(**vars(hp)).cuda().train())
    eager, graphed = models
    opt_e, opt_g = eager.configure_optimizers(), graphed.configure_optimizers()
    step = GraphedTrainStep(graphed, opt_g)
    img = torch.from_numpy(prng.uniform((B, 3, 64, 64), 7, 0.0, 1.0)).cuda()
    caps, lengths = prng.captions(B, R, T, 120, 8)
    batch = (img, torch.from_numpy(caps).cuda(), torch.from_numpy(lengths))
    for it in range(3):
        opt_e.zero_grad(set_to_none=True)
        out_e = eager.training_step(batch, it)
        out_e["loss"].backward()
        opt_e.step()
        out_g = step(batch, it)
        assert torch.equal(out_e["loss"].detach(), out_g["loss"]), (it, float(out_e["loss"]), float(out_g["loss"]))
    assert step.stats["eager: dropout"] == 3 and step.stats["replayed"] == 0 and step.stats["captured"] == 0, dict(step.stats)
