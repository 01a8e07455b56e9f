"""GPU: averaged weights in the fused optimizer step ("Averaged weights"; csrc/optimizer.hip) against torch's own optimizers
on the CPU (tests/averaging_ref.py): ``kind="asgd"`` is ``torch.optim.ASGD``, ``ema_decay`` is ``Tensor.lerp_`` after the step.  Also
the checkpoint interchange with torch, the swap, the fast path, reproducibility, the replayed (hipGraph) step and the unchanged default."""
import copy

import pytest
import torch

import averaging_ref as R

pytestmark = pytest.mark.gpu

CASES = [
    ("asgd", dict(lambd=1e-3, t0=2), None, None, None),                     # weight decay in the second group
    ("asgd", dict(lambd=0.0), ("norm", 0.5), None, 2),                      # the NT-ASGD recipe: start_averaging() after step 2
    ("adam", {}, None, 0.9, None),
    ("adamw", {}, ("value", 0.02), 0.9, None),
    ("sgd", {}, None, 0.5, None),                                           # momentum 0.9, nesterov
]


def _fused(kind, dev, kw, clip, ema):
    import sat_amd  # noqa: F401
    from sat_amd.optim import FusedOptimizer
    return FusedOptimizer(R.groups(dev), kind=kind, lr=1e-2, betas=(0.8, 0.95), momentum=0.9 if kind == "sgd" else 0.0, nesterov=kind == "sgd",
                          grad_clip=clip[0] if clip else None, clip_value=clip[1] if clip else 0.0, ema_decay=ema or 0.0, **kw)


def _give_grads(ref, dev, g, step):
    for p, q in zip(ref, dev):
        gr = torch.randn(p.shape, generator=g) * (0.1 if step % 2 else 1.0)
        p.grad = gr.clone(); q.grad = gr.cuda()


@pytest.mark.parametrize("kind,kw,clip,ema,average_after", CASES)
def test_averaged_step_matches_torch(kind, kw, clip, ema, average_after):
    ref, g = R.make_params()
    dev = R.device_twins(ref)
    topt = R.torch_optimizer(kind, R.groups(ref), **kw)
    fopt = _fused(kind, dev, kw, clip, ema)
    tema = R.Ema(ref, ema) if ema else None
    name = "ax" if kind == "asgd" else "ema"
    sched_t = torch.optim.lr_scheduler.ExponentialLR(topt, gamma=0.7)
    sched_f = torch.optim.lr_scheduler.ExponentialLR(fopt, gamma=0.7)
    for step in range(4):
        _give_grads(ref, dev, g, step)
        norm = R.clip(ref, clip)
        topt.step(); fopt.step()
        if tema:
            tema.update()
        if norm is not None:
            assert abs(float(fopt.last_grad_norm) - float(norm)) <= 1e-5 * float(norm)
        sched_t.step(); sched_f.step()
        if average_after is not None and step + 1 == average_after:
            assert fopt.start_averaging() == average_after
            for gr in topt.param_groups:
                gr["t0"] = average_after
        for i, (p, q) in enumerate(zip(ref, dev)):
            avg_ref = topt.state[p]["ax"] if kind == "asgd" else tema.avg[i]
            avg = fopt.state[q][name]
            R.within(q, p, "%s step %d p[%d]" % (kind, step, i))
            R.within(avg, avg_ref, "%s step %d %s[%d]" % (kind, step, name, i))
            if step == 0:
                assert torch.equal(avg, q.detach()), "the average must start as a copy of the parameter"
            if kind == "asgd":
                assert float(fopt.state[q]["mu"]) == float(topt.state[p]["mu"]) and float(fopt.state[q]["eta"]) == float(topt.state[p]["eta"])
                assert fopt.state[q]["eta"].dim() == 0 and fopt.state[q]["mu"].dim() == 0
        f = dev[-2]
        assert torch.equal(f._sat_bf16_shadow, f.detach().to(torch.bfloat16)) and f._sat_shadow_version == f._version
    if kind == "asgd":
        assert float(fopt.state[dev[0]]["mu"]) < 1.0                    # averaging did start within the four steps
    keys = {"asgd": {"step", "eta", "mu", "ax"}, "sgd": {"step", "momentum_buffer", "ema"}}.get(kind, {"step", "exp_avg", "exp_avg_sq", "ema"})
    for q in dev:
        assert set(fopt.state[q]) == keys and float(fopt.state[q]["step"]) == 4


def _persistent(dev):
    return [torch.empty_like(q) for q in dev]


def _step_both(ref, dev, bufs, g, topt, fopt, tema=None):
    for p, q, b in zip(ref, dev, bufs):
        gr = torch.randn(p.shape, generator=g)
        p.grad = gr.clone(); b.copy_(gr.cuda()); q.grad = b
    topt.step(); fopt.step()
    if tema:
        tema.update()


def test_torchs_asgd_checkpoint_loads_and_the_table_is_rebuilt():
    import sat_amd  # noqa: F401
    from sat_amd.optim import FusedOptimizer
    g = torch.Generator().manual_seed(9)
    shapes = [(70001,), (33, 17), (5,)]
    ref = [torch.randn(s, generator=g).requires_grad_() for s in shapes]
    dev = [p.detach().clone().cuda().requires_grad_() for p in ref]
    kw = dict(lr=1e-2, lambd=1e-3, alpha=0.75, t0=1, weight_decay=0.01)
    topt = torch.optim.ASGD(ref, **kw)
    fopt = FusedOptimizer(dev, kind="asgd", **kw)
    bufs = _persistent(dev)
    for _ in range(3):
        _step_both(ref, dev, bufs, g, topt, fopt)
    old = [fopt.state[q]["ax"] for q in dev]
    sd = copy.deepcopy(topt.state_dict())
    for st in sd["state"].values():
        for k in st:
            st[k] = st[k].cuda()                                        # a checkpoint read with map_location="cuda"
    fopt.load_state_dict(sd)
    for o in old:
        o.fill_(float("nan"))                                           # a table that still pointed here would average into NaN
    with torch.no_grad():
        for p, q in zip(ref, dev):
            q.copy_(p)                                                  # the weights of the checkpoint
    for q in dev:
        assert set(fopt.state[q]) == {"step", "eta", "mu", "ax"} and fopt.state[q]["ax"].is_cuda
    for step in range(2):
        _step_both(ref, dev, bufs, g, topt, fopt)
        for i, (p, q) in enumerate(zip(ref, dev)):
            R.within(q, p, "loaded step %d p[%d]" % (step, i))
            R.within(fopt.state[q]["ax"], topt.state[p]["ax"], "loaded step %d ax[%d]" % (step, i))
            assert float(fopt.state[q]["mu"]) == float(topt.state[p]["mu"]) and float(fopt.state[q]["eta"]) == float(topt.state[p]["eta"])
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in old)
    assert float(fopt.state[dev[0]]["step"]) == 5
    # and back: torch loads what the fused optimizer saved
    back = torch.optim.ASGD([p.detach().clone().requires_grad_() for p in ref], **kw)
    back.load_state_dict(fopt.state_dict())
    assert float(back.state[back.param_groups[0]["params"][0]]["eta"]) == float(topt.state[ref[0]]["eta"])


@pytest.mark.parametrize("kind,ema", [("asgd", None), ("adam", 0.9)])
def test_swap_exchanges_parameters_and_average(kind, ema):
    import sat_amd  # noqa: F401
    ref, g = R.make_params(seed=13)
    dev = R.device_twins(ref)
    frozen = torch.randn(300, generator=g).cuda().requires_grad_()      # never receives a gradient
    frozen0 = frozen.detach().clone()
    fopt = _fused(kind, dev + [frozen], dict(t0=0) if kind == "asgd" else {}, None, ema)
    name = "ax" if kind == "asgd" else "ema"
    with pytest.raises(RuntimeError):
        fopt.swap_averaged()                                            # before the first step
    for step in range(3):
        for q in dev:
            q.grad = torch.randn(q.shape, generator=g).cuda()
        fopt.step()
    p0 = [q.detach().clone() for q in dev]
    a0 = [fopt.state[q][name].clone() for q in dev]
    assert not torch.equal(p0[1], a0[1])                                # the average is not the parameter any more
    addr = [(q.data_ptr(), fopt.state[q][name].data_ptr()) for q in dev]
    f = dev[-2]

    def check(ps, avs):
        for q, p, a in zip(dev, ps, avs):
            assert torch.equal(q.detach(), p) and torch.equal(fopt.state[q][name], a)
        assert torch.equal(f._sat_bf16_shadow, f.detach().to(torch.bfloat16)) and f._sat_shadow_version == f._version
        assert torch.equal(frozen.detach(), frozen0) and name not in fopt.state.get(frozen, {})
        assert addr == [(q.data_ptr(), fopt.state[q][name].data_ptr()) for q in dev]        # contents move, tensors stay

    assert fopt.swap_averaged() is True
    check(a0, p0)
    with pytest.raises(RuntimeError):
        fopt.step()                                                     # stepping while the average sits in the parameters
    check(a0, p0)
    assert fopt.swap_averaged() is False
    check(p0, a0)
    with pytest.raises(KeyError):
        with fopt.averaged_weights():
            check(a0, p0)
            raise KeyError("inside")
    check(p0, a0)
    for q in dev:
        q.grad = torch.randn(q.shape, generator=g).cuda()
    fopt.step()                                                         # and the run goes on
    assert float(fopt.state[dev[0]]["step"]) == 4


@pytest.mark.parametrize("kind,ema", [("asgd", None), ("adam", 0.9)])
def test_fast_path_follows_a_replaced_average(kind, ema):
    import sat_amd  # noqa: F401
    from sat_amd.optim import FusedOptimizer
    g = torch.Generator().manual_seed(5)
    ref = [torch.randn(64, 8, 3, 3, generator=g).requires_grad_(), torch.randn(300, generator=g).requires_grad_(), torch.randn(65537, generator=g).requires_grad_()]
    dev = [p.detach().clone().cuda().requires_grad_() for p in ref]
    if kind == "asgd":
        topt = torch.optim.ASGD(ref, lr=1e-2, lambd=0.0, t0=2)
        fopt = FusedOptimizer(dev, kind="asgd", lr=1e-2, lambd=0.0, t0=2)
        tema = None
    else:
        topt = torch.optim.Adam(ref, lr=1e-2)
        fopt = FusedOptimizer(dev, kind="adam", lr=1e-2, ema_decay=ema)
        tema = R.Ema(ref, ema)
    name = "ax" if kind == "asgd" else "ema"
    bufs = _persistent(dev)
    seen = []
    for _ in range(4):
        _step_both(ref, dev, bufs, g, topt, fopt, tema)
        seen.append(getattr(fopt, "fast_path_steps", 0))
    assert seen == [0, 1, 2, 3], seen                                   # from the second step on the table on the device is reused
    st = fopt.state[dev[2]]
    old = st[name]; st[name] = old.clone(); old.fill_(float("nan"))
    _step_both(ref, dev, bufs, g, topt, fopt, tema)
    assert fopt.fast_path_steps == 3                                    # the slow path once
    _step_both(ref, dev, bufs, g, topt, fopt, tema)
    assert fopt.fast_path_steps == 4
    torch.cuda.synchronize()
    assert torch.isnan(old).all()
    for i, (p, q) in enumerate(zip(ref, dev)):
        R.within(q, p, "p[%d]" % i)
        R.within(fopt.state[q][name], topt.state[p]["ax"] if kind == "asgd" else tema.avg[i], "%s[%d]" % (name, i))


def test_averaged_step_is_bitwise_reproducible():
    import sat_amd  # noqa: F401
    from sat_amd.optim import FusedOptimizer
    outs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(3)
        ps = [torch.randn(100000, generator=g).cuda().requires_grad_(), torch.randn(257, 129, generator=g).cuda().requires_grad_()]
        opt = FusedOptimizer(ps, kind="adam", lr=1e-3, grad_clip="norm", clip_value=0.3, ema_decay=0.9)
        for _ in range(3):
            for p in ps:
                p.grad = torch.randn(p.shape, generator=g).cuda()
            opt.step()
        outs.append([p.detach().clone() for p in ps] + [opt.state[p]["ema"].clone() for p in ps])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert not torch.equal(outs[0][0], outs[0][2])


def test_default_step_is_untouched(monkeypatch):
    """Without averaging the optimizer launches what it launched before: ``sat_optimizer_step``, the old tables, the old state."""
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    from sat_amd.optim import FusedOptimizer

    def run():
        g = torch.Generator().manual_seed(21)
        ps = [torch.randn(70001, generator=g).cuda().requires_grad_(), torch.randn(33, 17, generator=g).cuda().requires_grad_()]
        opt = FusedOptimizer(ps, kind="adam", lr=1e-3)
        for _ in range(3):
            for p in ps:
                p.grad = torch.randn(p.shape, generator=g).cuda()
            opt.step()
        opt.prepare_device_step(ps[0].device)
        return opt, [p.detach().clone() for p in ps]

    opt, first = run()
    assert len(opt.device_buffers()) == 5
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in opt.state.values())
    lib = _lib.lib()
    calls = []
    plain = lib.sat_optimizer_step

    def refuse(*a):
        raise AssertionError("an averaging entry point was called by a step without averaging")

    def counted(*a):
        calls.append(1)
        return plain(*a)

    for name in ("sat_optimizer_step_avg", "sat_optimizer_step_avg_dev", "sat_optimizer_swap"):
        monkeypatch.setattr(lib, name, refuse)
    monkeypatch.setattr(lib, "sat_optimizer_step", counted)
    _, second = run()
    assert len(calls) == 3
    assert all(torch.equal(a, b) for a, b in zip(first, second))


# ---------------------------------------------------------------------------------------------------------------- the replayed step
def _make(over, seed=42):
    """the small model of tests/test_gpu_graph.py"""
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    kw = dict(encoder_arch="resnet18", encoder_dim=64, input_size=64, encoder_size=3, vocab_size=120, embed_dim=24, attention_dim=16,
              decoder_dim=40, deep_output=True, weight_decay=0.0, decoder_lr=1e-3, embedding_lr=1e-2, encoder_lr=1e-4, opt="adam",
              adam_b1=0.9, adam_b2=0.999, momentum=0.9, nesterov=False, scheduler=None, decoder_tf="always", encoder_finetune_after=1,
              lr_warmup_steps=4)
    kw.update(over)
    hp = O.default_hparams(**kw)
    torch.manual_seed(seed)
    model = M.SAT(**vars(hp)).cuda().train()
    model.set_precision("bf16")
    return model, hp


def _batch(hp, seed, B=4, R_=3, T=9):
    from oracle import prng
    img = torch.from_numpy(prng.uniform((B, 3, hp.input_size, hp.input_size), seed, 0.0, 1.0))
    caps, lengths = prng.captions(B, R_, T, hp.vocab_size, seed + 1)
    return img.cuda(), torch.from_numpy(caps).cuda(), torch.from_numpy(lengths)


def _state(model, opt, name):
    out = [(k, v.detach().clone()) for k, v in model.state_dict().items() if torch.is_tensor(v)]
    n = 0
    for i, g in enumerate(opt.param_groups):
        for j, p in enumerate(g["params"]):
            st = opt.state.get(p, {})
            if st.get(name) is not None:
                out.append(("opt.%d.%d.%s" % (i, j, name), st[name].detach().clone())); n += 1
    return out, n


def _same(a, b, what):
    assert len(a) == len(b)
    for (k, x), (_, y) in zip(a, b):
        assert torch.equal(x, y), "%s: %s differs (max |d| = %.3e)" % (what, k, float((x.double() - y.double()).abs().max()))


def _equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_equal(a[k], b[k]) for k in a)
    return a == b


@pytest.mark.parametrize("over,name", [(dict(opt="adam", ema_decay=0.99), "ema"), (dict(opt="asgd", asgd_t0=3, asgd_lambd=0.0), "ax")])
def test_replayed_averaged_step_is_bit_equal_to_the_eager_one(over, name):
    from sat_amd.graph import GraphedTrainStep
    eager, hp = _make(over)
    graphed, _ = _make(over)
    opt_e, opt_g = eager.configure_optimizers(), graphed.configure_optimizers()
    assert opt_g.kind == over["opt"] and opt_g._avg_name == name
    step = GraphedTrainStep(graphed, opt_g)
    batches = [_batch(hp, 11), _batch(hp, 23)]
    for it in range(8):
        b = batches[it % 2]
        if it == 6:             # the averaged weights go into the parameters and back between two replays
            with eager.averaged_weights():
                cap_e = eager.caption(b[0], beamk=2)
            with graphed.averaged_weights():
                cap_g = graphed.caption(b[0], beamk=2)
            eager.train(); graphed.train()
            assert _equal(cap_e, cap_g)
        opt_e.zero_grad(set_to_none=True)
        out_e = eager.training_step(b, it)
        out_e["loss"].backward()
        opt_e.step()
        out_g = step(b, it)
        assert torch.equal(out_e["loss"].detach(), out_g["loss"]), "step %d: loss %r vs %r" % (it, float(out_e["loss"]), float(out_g["loss"]))
        se, ne = _state(eager, opt_e, name)
        sg, ng = _state(graphed, opt_g, name)
        assert ne == ng > 0
        _same(se, sg, "after step %d" % it)
    print(dict(step.stats))
    assert step.stats["replayed"] >= 4, dict(step.stats)
    p = opt_g.param_groups[0]["params"][0]
    assert not torch.equal(opt_g.state[p][name], p.detach())            # an average, not a copy
