"""GPU parity of the mobilenet_v3_small encoder (model.py:38-39): the depthwise 5x5 kernels, BatchNorm + hard-swish and squeeze-and-excitation
against torch on the CPU, one inverted residual in bf16 storage against the rounding emulation, and the whole get_encoder / train step against
the test restatement (tests/mobilenet_v3_ref.py) with the same weights.  torchvision's MobileNetV3 is third-party arithmetic absent from the
reference tree: parity is unpinned at the reference level and pinned structurally (tests/test_mobilenet_v3.py: 927,008 parameters, 576
features, dev/encoder_summaries.txt:40).  Every tolerance is the one of the existing test of the same arithmetic (test_gpu_shufflenet.py,
test_gpu_mobilenet.py)."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def close(a, b, tol, what=""):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    print("%s: max|d| %.3e (scale %.3g, bound %.1e)" % (what, err, scale, tol * scale))
    assert err <= tol * scale, "%s: max|d|=%.3e (scale %.3g)" % (what, err, scale)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2)


def l2(a, b):
    return float((a.detach().cpu().double() - b.detach().double()).norm() / max(1e-12, float(b.detach().double().norm())))


def _zero_gradient_keys(enc_or_ref):
    """The project BatchNorm of every inverted residual (no activation) feeds the next 1x1 convolution + train-mode BatchNorm (the next block's
    expansion, or the last 1x1), directly or through identity paths: a per-channel shift of its output is subtracted again, so the gradient
    of its bias is exactly zero and what any implementation computes there is rounding noise, measured against the same layer's weight."""
    feats = [m for m in enc_or_ref.children()][1]
    return {"1.%d.block.%d.1.bias" % (i, len(blk.block) - 1) for i, blk in enumerate(list(feats)[1:-1], 1)}


# ----------------------------------------------------------------------------- depthwise 5x5
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("N,H,W,C,stride", [(1, 1, 1, 8, 1), (1, 1, 1, 8, 2), (2, 7, 5, 8, 1), (3, 9, 13, 16, 2), (2, 6, 11, 24, 2),
                                             (8, 28, 28, 96, 2), (16, 14, 14, 240, 1), (8, 7, 7, 576, 1), (4, 14, 14, 288, 2), (32, 17, 16, 40, 1)])
def test_depthwise5x5_fwd_dgrad_wgrad(N, H, W, C, stride, dtype):
    """against torch.nn.Conv2d(groups=C) on the CPU (tolerances of test_gpu_shufflenet.py::test_depthwise3x3_fwd_dgrad_wgrad); the filter
    gradient is bit-identical when rerun (fixed-order finish).  (32, 17, 16): 8704 output rows."""
    import sat_amd  # noqa: F401
    from oracle import prng
    from sat_amd import encoder_mobilenet_v3 as M3
    bf = dtype == "bf16"
    rnd = (lambda t: t.to(torch.bfloat16).float()) if bf else (lambda t: t)
    x = rnd(torch.from_numpy(prng.uniform((N, C, H, W), 5)))
    conv = torch.nn.Conv2d(C, C, 5, stride, 2, bias=False, groups=C)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(prng.uniform((C, 1, 5, 5), 6)))
    xr = x.clone().requires_grad_(True)
    y_ref = conv(xr)
    dy = rnd(torch.from_numpy(prng.uniform(tuple(y_ref.shape), 7)))
    y_ref.backward(dy)
    adt = torch.bfloat16 if bf else torch.float32
    cg = copy.deepcopy(conv).cuda()
    xg = nhwc(x).cuda().to(adt)
    y = M3.dw5_fwd(xg, cg)
    assert y.dtype == adt
    tol = 1e-2 if bf else 1e-5
    close(nchw(y.float()), y_ref, tol, "depthwise 5x5 forward")
    dyg = nhwc(dy).cuda().to(adt)
    dx = M3.dw5_dgrad(dyg, cg, tuple(xg.shape))
    close(nchw(dx.float()), xr.grad, tol, "depthwise 5x5 data gradient")
    dw = M3.dw5_wgrad(dyg, xg, cg).clone()
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (C, 1, 5, 5)
    close(dw, conv.weight.grad, 2e-5, "depthwise 5x5 filter gradient")
    assert torch.equal(M3.dw5_wgrad(dyg, xg, cg), dw)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- BatchNorm + hard-swish
@pytest.mark.parametrize("N,H,W,C", [(4, 5, 5, 8), (2, 16, 16, 96), (8, 7, 7, 40), (3, 9, 9, 144)])
def test_batchnorm_hardswish_fwd_bwd_eval(N, H, W, C):
    """against BatchNorm2d(eps=1e-3, momentum=0.01) + F.hardswish with the tolerances of test_gpu_mobilenet.py::test_batchnorm_relu6_fwd_bwd:
    more than 1 % of the values in each of the regions v < -3, -3 <= v <= 3, v > 3; channel 0 has gamma 0, beta +3 (every v exactly 3) and
    channel 1 gamma 0, beta -3 (every v exactly -3).  torch's hardswish_backward takes the outer branch at both kinks (v <= -3 -> 0, v < 3 ->
    g (v / 3 + 0.5), else g): g at v = 3 and 0 at v = -3, which the two channels' dbeta pin exactly."""
    import sat_amd  # noqa: F401
    from sat_amd import encoder_mobilenet_v3 as M3
    g = torch.Generator().manual_seed(C + N)
    bn = torch.nn.BatchNorm2d(C, eps=0.001, momentum=0.01)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) * 3 + 2.0); bn.bias.copy_(torch.randn(C, generator=g))
        bn.weight[0] = 0.0; bn.bias[0] = 3.0; bn.weight[1] = 0.0; bn.bias[1] = -3.0
        bn.running_mean.uniform_(-0.5, 0.5, generator=g); bn.running_var.uniform_(0.5, 2.0, generator=g)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    x = (torch.randn(N, C, H, W, generator=g) * 2 + 0.5).requires_grad_()
    v = bn(x)
    y = F.hardswish(v)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    vd = v.detach()
    assert float((vd < -3).float().mean()) > 0.01 and float(((vd >= -3) & (vd <= 3)).float().mean()) > 0.01 and float((vd > 3).float().mean()) > 0.01
    assert bool((vd[:, 0] == 3).all()) and bool((vd[:, 1] == -3).all())
    bnd = torch.nn.BatchNorm2d(C, eps=0.001, momentum=0.01).cuda()
    with torch.no_grad():
        bnd.weight.copy_(bn.weight); bnd.bias.copy_(bn.bias); bnd.running_mean.copy_(rm0); bnd.running_var.copy_(rv0)
    xd = nhwc(x.detach()).cuda()
    yd, stats = M3.bn_hs_fwd(xd, bnd, True)
    close(nchw(yd), y, 1e-5, "bn + hardswish fwd")
    close(bnd.running_mean, bn.running_mean, 1e-5, "running_mean"); close(bnd.running_var, bn.running_var, 1e-5, "running_var")
    assert int(bnd.num_batches_tracked) == 1
    dx, dgam, dbet = M3.bn_hs_bwd(nhwc(dy).cuda(), xd, stats, bnd)
    close(nchw(dx), x.grad, 2e-5, "dx"); close(dgam, bn.weight.grad, 2e-5, "dgamma"); close(dbet, bn.bias.grad, 2e-5, "dbeta")
    assert float(bn.bias.grad[1]) == 0.0 and float(dbet[1]) == 0.0          # v = -3: no gradient
    close(dbet[:1], dy[:, 0].double().sum().reshape(1), 2e-5, "dbeta at v = 3")          # v = 3: slope 1
    bn.eval(); bnd.eval()
    yde, _ = M3.bn_hs_fwd(xd, bnd, False)
    close(nchw(yde), F.hardswish(bn(x.detach())), 1e-5, "eval")


# ----------------------------------------------------------------------------- squeeze-and-excitation
@pytest.mark.parametrize("N,C,H,W", [(4, 16, 14, 14), (3, 96, 7, 7), (2, 576, 3, 5), (5, 24, 1, 1), (8, 240, 14, 14), (2, 16, 56, 56)])
def test_squeeze_excitation_fwd_bwd(N, C, H, W):
    """against torch autograd of torchvision's SqueezeExcitation: output, input gradient and the four parameter gradients at 1e-5 (fp32).
    Channel 0 has an fc2 pre-activation of exactly +3 and channel 1 of exactly -3 (zero weight rows, bias +-3): hardsigmoid 1 and 0, and - as
    torch's hardsigmoid_backward, strict -3 < z < 3 - no gradient through them."""
    import sat_amd  # noqa: F401
    import mobilenet_v3_ref as R
    from oracle import prng
    from sat_amd import encoder_mobilenet_v3 as M3
    torch.manual_seed(C + N)
    se = R.SqueezeExcitationRef(C)
    with torch.no_grad():
        S = se.fc1.out_channels          # pre-activations of order 1: both ReLU and hardsigmoid regions are populated
        se.fc1.weight.copy_(torch.from_numpy(prng.uniform(tuple(se.fc1.weight.shape), 31)) * (2.0 / C ** 0.5))
        se.fc1.bias.copy_(torch.from_numpy(prng.uniform(tuple(se.fc1.bias.shape), 32)) * 0.5)
        se.fc2.weight.copy_(torch.from_numpy(prng.uniform(tuple(se.fc2.weight.shape), 33)) * (6.0 / S ** 0.5))
        se.fc2.bias.copy_(torch.from_numpy(prng.uniform(tuple(se.fc2.bias.shape), 34)) * 2.0)
        se.fc2.weight[0].zero_(); se.fc2.bias[0] = 3.0; se.fc2.weight[1].zero_(); se.fc2.bias[1] = -3.0
    x = (torch.from_numpy(prng.uniform((N, C, H, W), 35)) * 3 - 1.0).requires_grad_()
    z2 = se.fc2(se.relu(se.fc1(F.adaptive_avg_pool2d(x.detach(), 1))))
    assert bool((z2[:, 0] == 3).all()) and bool((z2[:, 1] == -3).all())
    y = se(x)
    dy = torch.from_numpy(prng.uniform(tuple(y.shape), 36))
    y.backward(dy)
    sg = copy.deepcopy(se).cuda()
    xd = nhwc(x.detach()).cuda()
    yd, rec = M3.se_fwd(xd, sg)
    close(nchw(yd), y, 1e-5, "SE forward")
    grads = {}
    dx = M3.se_bwd(nhwc(dy).cuda(), xd, rec, sg, grads)
    close(nchw(dx), x.grad, 1e-5, "SE dx")
    for name in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
        p = dict(sg.named_parameters())[name]
        close(grads[p].reshape(dict(se.named_parameters())[name].shape), dict(se.named_parameters())[name].grad, 1e-5, "SE d" + name)
    assert float(grads[sg.fc2.bias][:2].abs().max()) == 0.0


# ----------------------------------------------------------------------------- one block in bf16 storage
@pytest.mark.parametrize("cfg,nb,hw", [((16, 3, 16, 16, True, "RE", 2), 8, 28), ((24, 3, 88, 24, False, "RE", 1), 8, 28), ((24, 5, 96, 40, True, "HS", 2), 8, 28),
                                       ((40, 5, 240, 40, True, "HS", 1), 8, 14), ((48, 5, 144, 48, True, "HS", 1), 6, 9), ((48, 5, 288, 96, True, "HS", 2), 8, 14)])
def test_inverted_residual_bf16_storage(cfg, nb, hw):
    """One inverted residual in bf16 storage from identical bf16-exact inputs against the rounding emulation (tests/mobilenet_v3_ref.py), with
    and without SE, ReLU and hard-swish, with and without the identity path: output and input gradient within 1e-2 relative L2, parameter
    gradients within 3e-2 (test_gpu_mobilenet.py::test_inverted_residual_bf16_storage)."""
    import sat_amd  # noqa: F401
    import mobilenet_v3_ref as R
    from oracle import prng
    from sat_amd import encoder as E, encoder_mobilenet_v3 as M3
    torch.manual_seed(cfg[0] + cfg[6])
    ref = R.InvertedResidualRef(*cfg).train()
    with torch.no_grad():
        for mod in ref.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 2.5); mod.bias.uniform_(-0.3, 1.5)
    blk = M3.InvertedResidual(*cfg)
    blk.load_state_dict(ref.state_dict())
    blk = blk.cuda().train()
    x = R.bf(torch.from_numpy(prng.uniform((nb, cfg[0], hw, hw), 21))).requires_grad_(True)
    y_ref = R.block_forward(ref, x)
    dy = R.bf(torch.from_numpy(prng.uniform(tuple(y_ref.shape), 22)))
    y_ref.backward(dy)
    Wt = E._weight_reader(True)
    r, y = M3._block_fwd(blk, nhwc(x.detach()).cuda().to(torch.bfloat16), True, Wt)
    errs = {"out": l2(nchw(y.float()), y_ref)}
    grads = {}
    dx = M3._block_bwd(r, nhwc(dy).cuda().to(torch.bfloat16), grads, Wt)
    errs["dx"] = l2(nchw(dx.float()), x.grad)
    gref = dict(ref.named_parameters())
    for k, p in blk.named_parameters():
        errs[k] = l2(grads[p].reshape(gref[k].shape), gref[k].grad)
    print(errs)
    assert errs["out"] <= 1e-2 and errs["dx"] <= 1e-2, errs
    assert max(errs.values()) <= 3e-2, errs


# ----------------------------------------------------------------------------- the whole encoder
@pytest.mark.parametrize("es,px,D,nb", [(None, 224, None, 8), (3, 64, 32, 8), (14, 256, 512, 4)])
def test_whole_mobilenet_v3_encoder_against_oracle(es, px, D, nb):
    """fp32 parity mode, forward + every gradient + running statistics + eval mode against the CPU restatement; the criteria of
    test_gpu_mobilenet.py::test_whole_mobilenet_encoder_against_oracle (annotations 2e-4; every gradient's error to the fp64 oracle <= 2 x the
    fp32 CPU oracle's + 5e-3 / 2e-2 slack for one activation decision near a kink taken the other way)."""
    import mobilenet_v3_ref as R
    from oracle import prng, sat_oracle as O
    from sat_amd import encoder as E
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    hp = O.default_hparams(encoder_arch="mobilenet_v3_small", encoder_dim=D, input_size=px, encoder_size=es)
    torch.manual_seed(3)
    ref = R.build_encoder(hp)
    hp2 = O.default_hparams(encoder_arch="mobilenet_v3_small", encoder_dim=D, input_size=px, encoder_size=es)
    torch.manual_seed(3)
    enc = E.get_encoder(hp2)
    assert hp2.encoder_dim == hp.encoder_dim
    assert list(enc.state_dict().keys()) == list(ref.state_dict().keys())
    for k, v in enc.state_dict().items():
        assert torch.equal(v, ref.state_dict()[k]), k
    zero = _zero_gradient_keys(ref)
    enc = enc.cuda().train()
    img = torch.from_numpy(prng.uniform((nb, 3, px, px), 77, 0.0, 1.0))
    ref64 = copy.deepcopy(ref).double()
    y_ref = ref(img.clone())
    dy = torch.from_numpy(prng.uniform(tuple(y_ref.shape), 78))
    y_ref.backward(dy)
    y64 = ref64(img.double().clone()); y64.backward(dy.double())
    y = enc(img.cuda())
    assert y.shape == y_ref.shape
    close(y, y_ref, 2e-4, "annotations")
    y.backward(dy.cuda())
    gref = dict(ref.named_parameters()); g64 = dict(ref64.named_parameters())
    worst = (0.0, 0.0, "")
    for k, p in enc.named_parameters():
        assert p.grad is not None, k
        exact = g64[k].grad
        nrm = max(1e-12, float(exact.norm()))
        if k in zero:
            nrm = max(1e-12, float(g64[k[:-4] + "weight"].grad.norm()))
        err_gpu = float((p.grad.cpu().double() - exact).norm()) / nrm
        err_cpu = float((gref[k].grad.double() - exact).norm()) / nrm
        worst = max(worst, (err_gpu, err_cpu, k))
        slack = 5e-3 if px >= 128 else 2e-2
        assert err_gpu <= 2 * err_cpu + slack, "%s: HIP %.3e vs CPU-fp32 %.3e (relative L2 to fp64)" % (k, err_gpu, err_cpu)
    print("worst relative grad error vs fp64 (HIP, CPU fp32, tensor):", worst)
    sd, sr = enc.state_dict(), ref.state_dict()
    for k in sd:
        if "running" in k:
            close(sd[k], sr[k], 1e-4, k)
        if "num_batches" in k:
            assert int(sd[k]) == int(sr[k]), k
    enc.eval(); ref.eval()
    with torch.no_grad():
        close(enc(img.cuda()), ref(img.clone()), 2e-4, "eval annotations")


@pytest.mark.parametrize("es,px,D,nb", [(None, 224, None, 8), (7, 256, 256, 8)])
def test_whole_mobilenet_v3_encoder_bf16_storage_against_the_rounding_oracle(es, px, D, nb):
    """bf16 mode against the restatement that rounds to bf16 at the same storage points, with the relative criterion of
    test_gpu_mobilenet.py::test_whole_mobilenet_encoder_bf16_storage_against_the_rounding_oracle: annotations closer to the emulation than half
    the emulation's own distance from fp32 + 3e-2; gradients: the HIP path's error against the fp32 oracle <= twice the emulation's + 2e-2."""
    import mobilenet_v3_ref as R
    from oracle import prng, sat_oracle as O
    from sat_amd import encoder as E
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    hp = O.default_hparams(encoder_arch="mobilenet_v3_small", encoder_dim=D, input_size=px, encoder_size=es)
    torch.manual_seed(3)
    ref = R.build_encoder(hp)
    zero = _zero_gradient_keys(ref)
    enc = E.get_encoder(O.default_hparams(encoder_arch="mobilenet_v3_small", encoder_dim=D, input_size=px, encoder_size=es))
    enc.load_state_dict(ref.state_dict())
    enc = enc.cuda().train(); enc.precision = "bf16"
    img = torch.from_numpy(prng.uniform((nb, 3, px, px), 77, 0.0, 1.0))
    ref32 = copy.deepcopy(ref)
    y32 = ref32(img.clone())
    dy = R.bf(torch.from_numpy(prng.uniform(tuple(y32.shape), 78)))
    y32.backward(dy)
    y_ref = R.encoder_forward(ref, img)
    y_ref.backward(dy)
    y = enc(img.cuda())
    assert y.dtype == torch.float32
    ann_err, emu_cost = l2(y, y_ref), l2(y_ref, y32)
    print("bf16 mobilenet_v3 vs the rounding oracle: annotations relative L2", ann_err, " (emulation vs fp32:", emu_cost, ")")
    assert ann_err <= 0.5 * emu_cost + 3e-2
    y.backward(dy.cuda())
    gemu, g32 = dict(ref.named_parameters()), dict(ref32.named_parameters())
    for k, p in enc.named_parameters():
        if k in zero:
            assert float(p.grad.norm()) <= 4 * float(gemu[k].grad.norm()) + 1e-3 * float(gemu[k[:-4] + "weight"].grad.norm()), k
    rows = sorted(((l2(p.grad, g32[k].grad) - 2 * l2(gemu[k].grad, g32[k].grad), l2(p.grad, g32[k].grad), l2(gemu[k].grad, g32[k].grad), l2(p.grad, gemu[k].grad), k)
                   for k, p in enc.named_parameters() if k not in zero), reverse=True)
    print("bf16 mobilenet_v3: (HIP vs fp32, emulation vs fp32, HIP vs emulation) worst margins", [(round(a, 4), round(b, 4), round(c, 4), k) for _, a, b, c, k in rows[:4]])
    assert rows[0][0] <= 2e-2, rows[:4]
    sd, sr = enc.state_dict(), ref.state_dict()
    for k in sd:
        if "running" in k:
            close(sd[k], sr[k], 2e-2, k)
        if "num_batches" in k:
            assert int(sd[k]) == int(sr[k]), k


# ----------------------------------------------------------------------------- the whole train step behind the reference's SAT surface
def _make_model(monkeypatch, over=None, seed=42):
    import sat_amd  # noqa: F401
    import mobilenet_v3_ref as R
    from sat_amd import model as M
    from oracle import sat_oracle as O
    monkeypatch.setattr(O, "build_encoder", R.build_encoder)          # OracleSAT looks it up at call time
    kw = dict(encoder_arch="mobilenet_v3_small", encoder_dim=None, input_size=64, encoder_size=None, vocab_size=120, embed_dim=24,
              attention_dim=16, decoder_dim=40, deep_output=True, weight_decay=0.0, decoder_lr=1e-3, embedding_lr=1e-2,
              encoder_lr=1e-4, opt="adam", adam_b1=0.9, adam_b2=0.999, momentum=0.9, nesterov=False, scheduler=None)
    kw.update(over or {})
    hp = O.default_hparams(**kw)
    torch.manual_seed(seed)
    model = M.SAT(**vars(hp))
    oracle = O.OracleSAT(O.default_hparams(**kw), {k: v.clone() for k, v in model.state_dict().items()})
    return model.cuda().train(), oracle, hp


def _batch(hp, B=6, R=3, T=9, seed=5):
    from oracle import prng
    img = torch.from_numpy(prng.uniform((B, 3, hp.input_size, hp.input_size), seed, 0.0, 1.0))
    caps, lengths = prng.captions(B, R, T, hp.vocab_size, seed + 1)
    return img, torch.from_numpy(caps), torch.from_numpy(lengths)


@pytest.mark.parametrize("eps,D", [(1.0, None), (0.0, 32)])
def test_training_step_with_the_mobilenet_v3_encoder_matches_oracle(monkeypatch, eps, D):
    """SAT(encoder_arch="mobilenet_v3_small") - no projection (encoder_dim = 576) and the projected variant - one training_step against OracleSAT:
    loss 1e-4, accuracy, packed logits, attention maps, every gradient (test_gpu_mobilenet.py::test_training_step_with_the_mobilenet_encoder_matches_oracle)."""
    model, oracle, hp = _make_model(monkeypatch, dict(encoder_dim=D, decoder_tf="always" if eps == 1.0 else None))
    assert model.hp.encoder_dim == (576 if D is None else D)
    img, caps, lengths = _batch(hp)
    loss_o, out_o = oracle.step_loss(img, caps, lengths, eps)
    loss_o.backward()
    img_g = img.cuda()
    metrics = model.training_step((img_g, caps.cuda(), lengths), 0)
    assert torch.equal(img_g.cpu(), img)
    assert abs(metrics["loss"].item() - loss_o.item()) <= 1e-4 * max(1.0, abs(loss_o.item()))
    assert abs(float(metrics["accuracy"]) - float(out_o["acc"])) < 1e-6
    lp, tp, alphas = model.train_batch((img_g, caps.cuda(), lengths), eps)
    rel = lambda a, b: float((a.detach().cpu().double() - b.detach().double()).abs().max()) / max(1.0, float(b.detach().double().abs().max()))   # noqa: E731
    assert rel(lp.data, out_o["logits_packed"]) <= 2e-4 and rel(alphas, out_o["alphas"]) <= 1e-4
    metrics["loss"].backward()
    og = oracle.named_grads()
    zero = {"encoder." + k for k in _zero_gradient_keys(oracle.encoder)}
    worst = (0.0, "")
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        ref = og[k].double()
        nrm = float(og[k[:-4] + "weight"].double().norm()) if k in zero else float(ref.norm())
        e = float((p.grad.cpu().double() - ref).norm()) / max(1e-9, nrm)
        worst = max(worst, (e, k))
        assert e <= 2e-2, "%s: relative L2 gradient error %.3e" % (k, e)
    print("worst gradient error", worst)


def test_replayed_step_with_the_mobilenet_v3_encoder_is_bit_equal_to_the_eager_step(monkeypatch):
    """sat_amd/graph.py with the mobilenet_v3_small encoder in bf16 mode: over 7 steps the step replayed from a hipGraph leaves the same loss,
    parameters, BatchNorm buffers and optimizer moments as the eager loop, bit for bit."""
    from sat_amd.graph import GraphedTrainStep
    over = dict(decoder_tf="always", lr_warmup_steps=3)
    eager, _, hp = _make_model(monkeypatch, over)
    graphed, _, _ = _make_model(monkeypatch, over)
    eager.set_precision("bf16"); graphed.set_precision("bf16")
    eager.configure_optimizers(); graphed.configure_optimizers()
    opt_e, opt_g = eager._train_optimizer(), graphed._train_optimizer()
    step = GraphedTrainStep(graphed, opt_g)
    batches = []
    for seed in (11, 23):
        img, caps, lengths = _batch(hp, B=4, seed=seed)
        batches.append((img.cuda(), caps.cuda(), lengths))
    for it in range(7):
        b = batches[it % 2]
        opt_e.zero_grad(set_to_none=True)
        out_e = eager.training_step(b, it)
        out_e["loss"].backward()
        opt_e.step()
        out_g = step(b, it)
        assert torch.equal(out_e["loss"].detach(), out_g["loss"]), "step %d: loss %r vs %r" % (it, float(out_e["loss"]), float(out_g["loss"]))
        for (k, x), (_, y) in zip(eager.state_dict().items(), graphed.state_dict().items()):
            assert torch.equal(x, y), "step %d: %s differs" % (it, k)
    assert step.stats["captured"] >= 2 and step.stats["replayed"] >= 3, dict(step.stats)


def test_mobilenet_v3_steps_at_the_cli_defaults_are_reproducible_bit_for_bit():
    """The reference CLI's defaults (224 px, no projection, decoder_tf None, plain output layer) with 32 images x 5 captions in bf16 mode,
    trainable encoder: two identical models stepped twice on the same batch agree bit for bit in loss, every gradient and every updated tensor,
    recycled device memory poisoned with NaN in between; losses finite and near ln(V) at the start; gradients finite."""
    import math
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    hp, T, B, R = bench.hparams("cli")
    hp.update(encoder_arch="mobilenet_v3_small", decoder_tf=None, deep_output=False)
    img, caps, lengths = bench.synthetic_batch(B, R, T, hp["vocab_size"], 1234, True, px=hp["input_size"])
    img, caps = img.cuda(), caps.cuda()

    def run():
        torch.manual_seed(42)
        model = M.SAT(**hp).cuda().train(); model.set_precision("bf16")
        model.__dict__["_sat_global_step"] = 2
        opt = model.configure_optimizers()
        losses = []
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            out = model.training_step((img.clone(), caps, lengths), 0)
            out["loss"].backward()
            grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
            opt.step()
            losses.append(out["loss"].detach().clone())
        return losses, grads, {k: v.detach().clone() for k, v in model.state_dict().items()}

    l1, g1, s1 = run()
    junk = torch.full((1 << 26,), float("nan"), device="cuda"); del junk           # recycled blocks now hold NaN
    l2_, g2, s2 = run()
    assert all(torch.equal(a, b) for a, b in zip(l1, l2_)), (l1, l2_)
    assert [k for k in g1 if not torch.equal(g1[k], g2[k])] == []
    assert [k for k in s1 if not torch.equal(s1[k], s2[k])] == []
    assert all(math.isfinite(float(l)) for l in l1) and abs(float(l1[0]) - math.log(hp["vocab_size"])) < 1.0
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())
    assert sum(k.startswith("encoder.") for k in g1) == 138          # every trunk parameter has a gradient
