"""GPU: temperature-scaling calibration (sat_amd/calibration.py on csrc/temperature.hip) against the CPU restatement of the
reference's temperature_scaling.py:51-59 (tests/temperature_ref.py; float64 = the truth, float32 = the reference as it was run).

Bounds.  Fits: with e_ref32 = max|trace_float32 - trace_float64| of the restatement on the same input and e_hip = max|trace_hip -
trace_float64|, e_hip <= 2 * e_ref32 + ulp, ulp = 2^-23 * max(trace) -- the form tests/test_gpu_train_step.py uses: "no worse
than the same arithmetic in the same precision done in another order", plus one fp32 step of a value that is stored in fp32.
Single evaluations (nll_at): worst-case fp32 rounding of what the kernel computes per row -- a sum of V terms accumulated as
ceil(V / 64) sequential additions per lane and a 6-level butterfly, the exponent's product (< 1 unit), v_exp_f32 (1 unit), the
logarithm, the two divisions and the subtraction of each row term, the final rounding to fp32 (together < 16 units) -- i.e.
(ceil(V / 64) + 16) * 2^-24 of the largest per-row magnitude that enters the result, taken from the float64 restatement:
max_i(|x_iy - m_i| / T + log s_i + 1) for the loss (a relative error of s_i is an absolute error of log s_i) and max_i(|x_iy - m_i| + |sum_j p_ij (x_ij - m_i)|) / T^2 for the derivative.  The float64 restatement
works on the unshifted x / T, so its own rounding, 8 * 2^-53 * max|x| / T (/ T^2), is added: it matters at the offset of 1e4."""
import math

import pytest
import torch

import temperature_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EIGHT = [0.25, 0.5, 0.7, 1.0, 1.5, 2.0, 3.0, 4.0]


def cal():
    import sat_amd  # noqa: F401
    from sat_amd import calibration
    return calibration


def nll_scales(x, y, T):
    xd = x.double()
    m = xd.max(dim=1, keepdim=True).values
    d = xd - m
    e = torch.exp(d / T)
    s = e.sum(dim=1)
    xt = (xd.gather(1, y[:, None]) - m)[:, 0]
    loss_scale = float((xt.abs() / T + torch.log(s) + 1.0).max())          # + 1: a relative error of s is an absolute error of log s
    grad_scale = float((xt.abs() + ((d * e).sum(dim=1) / s).abs()).max()) / (T * T)
    ref_err = 8 * 2.0 ** -53 * float(xd.abs().max())          # the float64 restatement's own rounding: it works on x / T unshifted
    return max(loss_scale, 2.0 ** -20), max(grad_scale, 2.0 ** -20), ref_err / T, ref_err / (T * T)


def make_logits(kind, P, V, seed):
    if kind == "plain":
        return R.confident_logits(P, V, seed)
    if kind == "offset":                       # a large common offset per row: only the max-shifted form stays finite in fp32
        x, y = R.confident_logits(P, V, seed)
        return x + 1e4, y
    x, y = R.confident_logits(P, V, seed, boost=90.0, wrong=0.3, scale=60.0)          # "wide": row range >= 200, i.e. >= 800 at T = 0.25
    if V >= 97:
        assert float((x.max(dim=1).values - x.min(dim=1).values).min()) >= 200.0
    return x, y


@pytest.mark.parametrize("kind", ["plain", "offset", "wide"])
@pytest.mark.parametrize("P,V", [(1, 97), (7, 97), (301, 6400), (130, 10000), (2048, 1000), (5, 4), (3, 1)])
def test_nll_at_matches_float64(P, V, kind):
    """V % 4 != 0 (97), 6400, 10000, P = 1, P not a multiple of the 4 rows of a workgroup (7, 301, 130, 5, 3), 1 and 8 temperatures
    in one call (T from 0.25 to 4); 8 temperatures in one call equal 8 single calls bit for bit"""
    x, y = make_logits(kind, P, V, seed=100 + P + V)
    check_nll_at(x, y, x.to(DEV), y.to(DEV), kind)


def check_nll_at(x, y, xg, yg, kind):
    """nll_at on the device tensors xg, yg (the host tensors x, y) at 8 temperatures against the float64 restatement, within the bound of
    the module docstring"""
    C = cal()
    P, V = x.shape
    loss8, grad8 = C.nll_at(xg, yg, EIGHT)
    assert loss8.shape == (8,) and grad8.shape == (8,) and loss8.dtype == torch.float32 and loss8.is_cuda
    worst = 0.0
    for i, T in enumerate(EIGHT):
        loss1, grad1 = C.nll_at(xg, yg, [T])
        assert torch.equal(loss1, loss8[i:i + 1]) and torch.equal(grad1, grad8[i:i + 1]), "T=%g: one call of 8 differs from a single call" % T
        lr, gr = R.nll(x, y, T, torch.float64)
        ls, gs, rl, rg = nll_scales(x, y, T)
        units = (math.ceil(V / 64) + 16) * 2.0 ** -24
        bl, bg = units * ls + rl, units * gs + rg
        el, eg = abs(float(loss1) - lr), abs(float(grad1) - gr)
        print("P=%d V=%d %s T=%g: loss %.7g (ref %.7g) err %.2e / bound %.2e; dloss/dT %.7g (ref %.7g) err %.2e / bound %.2e"
              % (P, V, kind, T, float(loss1), lr, el, bl, float(grad1), gr, eg, bg))
        assert math.isfinite(float(loss1)) and math.isfinite(float(grad1))
        assert el <= bl and eg <= bg
        worst = max(worst, el / bl, eg / bg)
    print("P=%d V=%d %s: worst err / bound = %.3f" % (P, V, kind, worst))


@pytest.mark.parametrize("P,V", [(3, 1028), (7, 97), (5, 4)])
def test_nll_at_with_logits_off_their_alignment(P, V):
    """the logits start one float past a 16-byte boundary, so the rows take the 4-byte sweep whatever V is: V % 4 == 0 on that form
    (1028: 257 16-byte units when aligned, one lane's second load) is run by nothing else.  The aligned call gives the same row maxima
    and sums in another order, so both are held to the same bound."""
    x, y = make_logits("plain", P, V, seed=100 + P + V)
    buf = torch.empty(P * V + 4, dtype=torch.float32, device=DEV)
    xg = buf[1:1 + P * V].view(P, V)
    xg.copy_(x)
    assert buf.data_ptr() % 16 == 0 and xg.data_ptr() % 16 == 4 and xg.is_contiguous()
    check_nll_at(x, y, xg, y.to(DEV), "plain, logits one float off")
    check_nll_at(x, y, x.to(DEV), y.to(DEV), "plain, aligned")


def test_nll_at_accepts_more_than_eight_and_rejects_bad_input():
    C = cal()
    from sat_amd import _lib
    x, y = R.confident_logits(64, 97, 5)
    xg, yg = x.to(DEV), y.to(DEV)
    temps = [0.3 + 0.1 * i for i in range(11)]
    loss, grad = C.nll_at(xg, yg, temps)
    for i in (0, 7, 8, 10):
        l1, g1 = C.nll_at(xg, yg, [temps[i]])
        assert torch.equal(l1, loss[i:i + 1]) and torch.equal(g1, grad[i:i + 1])
    with pytest.raises(ValueError):
        C.nll_at(xg, yg, [1.0, 0.0])
    with pytest.raises(ValueError):
        C.nll_at(xg, yg, [])
    bad = yg.clone(); bad[3] = 97
    with pytest.raises(ValueError):
        C.nll_at(xg, bad, [1.0])
    with pytest.raises(ValueError):
        C.fit_temperature(xg, -yg - 1)
    with pytest.raises(_lib.SatHipError):
        C.fit_temperature(xg, yg, iters=0)
    with pytest.raises(_lib.SatHipError):
        C.fit_temperature(xg, yg, init=-1.0)
    with pytest.raises(_lib.SatHipError):
        C.fit_temperature(x, y)


CASES = {"v1000_right": (2048, 1000, 1, dict(boost=8.0, wrong=0.1)),             # T falls from 1.5 to 0.7 and comes back to 0.8
         "v1000_wrong": (2048, 1000, 2, dict(boost=12.0, wrong=0.5)),            # T rises to 1.7
         "v6400": (1024, 6400, 3, dict(boost=14.0, wrong=0.35, scale=2.0))}
VARIANTS = {"reference": {}, "plain_momentum": dict(nesterov=False), "no_momentum": dict(momentum=0.0, nesterov=False),
            "init2_iters40": dict(init=2.0, iters=40)}


def check_fit(fit, x, y, kw, what):
    t64, l64, _ = R.fit(x, y, dtype=torch.float64, **kw)
    t32, l32, _ = R.fit(x, y, dtype=torch.float32, **kw)
    assert float(t64.max() - t64.min()) >= 0.05, "%s: the temperature never moved in the float64 restatement" % what
    assert fit.trace.shape == t64.shape and fit.losses.shape == l64.shape
    assert float(fit.trace[0]) == kw["init"] and fit.temperature == float(fit.trace[-1])
    e_t, lim_t, ref_t = R.bound(fit.trace, t64, t32)
    e_l, lim_l, ref_l = R.bound(fit.losses, l64, l32)
    print("%s: T %.7f (float64 %.7f)  trace e_hip %.2e e_ref32 %.2e bound %.2e ratio e_hip/e_ref32 %.2f | loss e_hip %.2e e_ref32 %.2e bound %.2e ratio %.2f"
          % (what, fit.temperature, float(t64[-1]), e_t, ref_t, lim_t, e_t / max(ref_t, 1e-30), e_l, ref_l, lim_l, e_l / max(ref_l, 1e-30)))
    assert e_t <= lim_t, "%s: T trace e_hip %.3e > 2 * %.3e + ulp" % (what, e_t, ref_t)
    assert e_l <= lim_l, "%s: loss trace e_hip %.3e > 2 * %.3e + ulp" % (what, e_l, ref_l)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", list(CASES))
def test_fit_matches_restatement(case, variant):
    C = cal()
    P, V, seed, mix = CASES[case]
    x, y = R.confident_logits(P, V, seed, **mix)
    kw = dict(R.REFERENCE); kw.update(VARIANTS[variant])
    fit = C.fit_temperature(x.to(DEV), y.to(DEV), **kw)
    check_fit(fit, x, y, kw, "%s/%s" % (case, variant))


def test_fit_is_deterministic_and_stream_independent():
    C = cal()
    x, y = R.confident_logits(1030, 1000, 7)
    xg, yg = x.to(DEV), y.to(DEV)
    a = C.fit_temperature(xg, yg)
    b = C.fit_temperature(xg, yg)
    assert torch.equal(a.trace, b.trace) and torch.equal(a.losses, b.losses)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = C.fit_temperature(xg, yg)
    side.synchronize()
    assert torch.equal(a.trace, c.trace) and torch.equal(a.losses, c.losses)
    l1, g1 = C.nll_at(xg, yg, EIGHT)
    l2, g2 = C.nll_at(xg, yg, EIGHT)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_fit_latches_a_non_positive_temperature():
    """lr = 0.5 drives T below zero in the float64 restatement; the fit raises, T stays where it was caught, and the trace up to the
    offending step matches"""
    C = cal()
    from sat_amd import _lib
    x, y = R.confident_logits(2048, 1000, 1)
    kw = dict(R.REFERENCE); kw.update(lr=0.5, iters=12)
    t64, l64, _ = R.fit(x, y, dtype=torch.float64, **kw)
    t32, l32, _ = R.fit(x, y, dtype=torch.float32, **kw)
    k = int((t64 <= 0).nonzero()[0])
    assert k >= 1
    with pytest.raises(_lib.SatHipError) as info:
        C.fit_temperature(x.to(DEV), y.to(DEV), **kw)
    trace, losses = info.value.trace, info.value.losses
    assert trace.shape == (13,) and losses.shape == (12,)
    e_t, lim_t, _ = R.bound(trace[:k + 1], t64[:k + 1], t32[:k + 1])
    e_l, lim_l, _ = R.bound(losses[:k], l64[:k], l32[:k])
    print("latched at step %d: T %.6f (float64 %.6f); e_hip %.2e bound %.2e; loss e_hip %.2e bound %.2e" % (k, float(trace[k]), float(t64[k]), e_t, lim_t, e_l, lim_l))
    assert e_t <= lim_t and e_l <= lim_l
    assert float(trace[k]) <= 0
    assert bool((trace[k:] == trace[k]).all()), "T moved after the latch"
    assert bool(torch.isnan(losses[k:]).all())


def tiny_model(precision="fp32"):
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=97, embed_dim=24,
                attention_dim=16, decoder_dim=40, deep_output=True, decoder_tf="always")
    torch.manual_seed(42)
    model = M.SAT(**vars(O.default_hparams(**over))).to(DEV)
    with torch.no_grad():          # a freshly initialised model is indifferent (logits within +-1.5): sharpen it so that calibration has work to do
        model.output.output.weight.mul_(8.0)
        model.output.output.bias.mul_(8.0)
    model.set_precision(precision)
    return model


def tiny_batches(n):
    from oracle import prng
    out = []
    for i in range(n):
        img = torch.from_numpy(prng.uniform((4, 3, 64, 64), 60 + i, 0.0, 1.0))
        caps, lengths = prng.captions(4, 3, 9, 97, 70 + i)
        out.append((img, torch.from_numpy(caps), torch.from_numpy(lengths)))
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_calibrate_temperature_end_to_end(precision):
    """model.calibrate_temperature(batches) = the restatement fed with the concatenated train_batch(epsilon=1) logits of the same
    model in eval mode (fp32 logits in both precision modes); state_dict and train/eval mode unchanged"""
    model = tiny_model(precision).train()
    batches = tiny_batches(4)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    hp_before = dict(model.hp)
    fit = model.calibrate_temperature(batches)
    assert model.training
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert dict(model.hp) == hp_before
    model.eval()
    xs, ys = [], []
    with torch.no_grad():
        for img, caps, lengths in batches:
            lp, tp, _ = model.train_batch((img.to(DEV), caps.to(DEV), lengths), epsilon=1)
            assert lp.data.dtype == torch.float32
            xs.append(lp.data.cpu()); ys.append(tp.data.cpu())
    x, y = torch.cat(xs), torch.cat(ys)
    assert math.isfinite(fit.temperature) and fit.temperature > 0
    check_fit(fit, x, y, dict(R.REFERENCE), "end to end %s (P=%d)" % (precision, x.shape[0]))
    model.eval()
    fit2 = model.calibrate_temperature(batches, max_batches=2, iters=10)
    assert not model.training and fit2.trace.shape == (11,)


def test_collect_logits_order_and_max_batches():
    C = cal()
    model = tiny_model().eval()
    batches = tiny_batches(3)
    per = []
    with torch.no_grad():
        for img, caps, lengths in batches:
            lp, tp, _ = model.train_batch((img.to(DEV), caps.to(DEV), lengths), epsilon=1)
            per.append((lp.data, tp.data))
    x, y = C.collect_logits(model, batches)
    assert torch.equal(x, torch.cat([p[0] for p in per])) and torch.equal(y, torch.cat([p[1] for p in per]))
    x2, y2 = C.collect_logits(model, batches, max_batches=2)
    assert torch.equal(x2, torch.cat([p[0] for p in per[:2]])) and torch.equal(y2, torch.cat([p[1] for p in per[:2]]))
    x1, _ = C.collect_logits(model, iter(batches), max_batches=1)
    assert x1.shape[0] == per[0][0].shape[0]
    # the PackedSequence pair of train_batch goes in as it is
    with torch.no_grad():
        lp, tp, _ = model.train_batch((batches[0][0].to(DEV), batches[0][1].to(DEV), batches[0][2]), epsilon=1)
    la, ga = C.nll_at(lp, tp, [1.5])
    lb, gb = C.nll_at(lp.data, tp.data, [1.5])
    assert torch.equal(la, lb) and torch.equal(ga, gb)
