"""GPU: the token losses ("Token losses") against their float64 specification (tests/token_loss_ref.py) and the CPU oracle:
the kernels (csrc/token_loss.hip) through the C ABI with every output inside a guard band, then ``token_loss`` / ``focal_gamma`` /
``ul_alpha`` inside the train step.

Tolerances.  The kernels: tests/test_gpu_distill.py's, 5e-6 of the largest reference entry (floored at 1) for every array, gradient
included (gscale is 1.7 P, so the largest gradient entry is O(1) and the floor does not hide it), and 5e-6 of the sum of the magnitudes
of its terms (floored at 1) for each mean; the accuracy exactly.  The regular cases are drawn so that the reference is well
conditioned in 1 - p_c (``case`` says why and how).  The whole step: exactly the bounds of
tests/test_gpu_train_step.py::test_training_step_matches_oracle.

Measured on an MI355X: the kernel arrays within 3.0e-7 on a scale of 1 (ul rows, gradients) and 3.0e-6 on a scale of 20 (fl rows at
gamma = 5); the step's loss within 1e-7 relative, its four metrics within 2e-7, the worst parameter gradient 1.1e-5 relative L2."""
import functools

import numpy as np
import pytest
import torch

import token_loss_ref as R
from test_gpu_distill import TOL, Banded, close, rows

pytestmark = pytest.mark.gpu

PAD = 0
SHAPES = [(3, 4, 8, 5), (2, 5, 7, 5), (5, 9, 1003, 5), (4, 12, 4100, 5), (3, 9, 10000, 5), (6, 42, 4100, 5), (6, 42, 4100, 40)]      # N, T, V, W
WEIGHTS = [(1.0, 0.0, 2.0, 1.0, 0.1), (0.0, 1.0, 2.0, 0.0, 0.0), (1.0, 1.0, 0.5, 0.5, 0.0), (1.0, 1.0, 5.0, 2.0, 0.1), (0.0, 0.0, 2.0, 1.0, 0.0)]
#          ce_weight, focal_weight, gamma, ul_alpha, smoothing


MIN_MEAN_UL = 0.05
# What one ulp of an lse between 8 and 16 (2^-20) may do to a candidate's gradient entry ul_alpha g / P r_c, r_c = p_c / (1 - p_c), through
# d r_c / d lse = p_c / (1 - p_c)^2, held inside TOL of the array's scale.  The strictest weight set is the unlikelihood alone (ul_alpha
# 1, g / P = 1.7, scale = the floor 1); the heaviest (ul_alpha 2) has the target's entry g / P (1 - smoothing + w) ~ 3 as its scale.
MAX_CONDITION = TOL / (1.0 * 1.7 * 2.0 ** -20)


def condition(z, cand):
    """per row, max_c p_c / (1 - p_c)^2 on the float64 reference (0 for a row without candidates); also the rows' ul"""
    logp = torch.log_softmax(z.double(), dim=1)
    kappa, ul = torch.zeros(len(cand), dtype=torch.float64), torch.zeros(len(cand), dtype=torch.float64)
    for p, c in enumerate(cand):
        if c:
            om = -torch.expm1(logp[p, torch.tensor(c)])
            kappa[p], ul[p] = ((1.0 - om) / om ** 2).max(), -om.log().sum()
    return kappa, ul


def draw_case(N, T, V, W, seed):
    """ragged captions (one of full length) whose words come from W distinct ids, so that contexts repeat; logits as test_gpu_distill.py's
    ``rows`` plus 6.0 on each row's context ids (without the lift the candidates' mass, and the unlikelihood with it, vanishes under
    the tolerance floor at a large V).  A row whose reference is ill conditioned (see ``case``) is drawn again, alone."""
    from oracle import prng
    lengths = torch.from_numpy(prng.integers((N,), seed, 2, T))
    lengths[0] = T - 1
    step = max(1, (V - 3) // W)
    ids = torch.tensor([1 + k * step for k in range(W)])
    draws = torch.from_numpy(prng.integers((N, T), seed + 1, 0, W))
    caps = torch.zeros(N, T, dtype=torch.int64)
    for i in range(N):
        n = int(lengths[i])
        caps[i, 0] = V - 2
        caps[i, 1:n] = ids[draws[i, 1:n]]
        caps[i, n] = V - 1
    caps[0, 2] = caps[0, 1]                      # the full-length caption says its first word twice, whatever was drawn
    cand, y = R.candidates(caps, lengths, V, PAD)
    cap, stp = R.packed_steps(lengths, T)
    P = len(cand)
    lift = torch.zeros(P, V)
    repeats = False
    for p, (i, t) in enumerate(zip(cap.tolist(), stp.tolist())):
        ctx = [int(c) for c in caps[i, 1:t + 1] if 0 <= int(c) < V]
        repeats = repeats or len(set(ctx)) < len(ctx)
        if ctx:
            lift[p, torch.tensor(sorted(set(ctx)))] = 6.0
    assert repeats, "no row has two equal context ids"
    z = rows(P, V, 1, seed + 2)[0] + lift
    for k in range(1, 40):
        kappa, ul = condition(z, cand)
        bad = kappa > MAX_CONDITION
        if not bool(bad.any()):
            break
        z[bad] = (rows(P, V, 1, seed + 2 + 7 * k)[0] + lift)[bad]
    return dict(caps=caps, lengths=lengths, cand=cand, y=y, z=z, src=R.src_rows(lengths, T), P=P, N=N, T=T, V=V, seed=seed, condition=float(kappa.max()),
                mean_ul=float(ul.mean()))


@functools.lru_cache(maxsize=None)
def case(N, T, V, W):
    """The first draw (seeds 700 + N + T + W, + 100, + 200, ...) whose REFERENCE is a regular case: mean ul >= 0.05, so that the term is
    far above the tolerance floor, and in every row max_c p_c / (1 - p_c)^2 <= MAX_CONDITION (about 3: no 1 - p_c below 0.43).  The
    second is a matter of the number format, not of the kernels.  They take 1 - p_c as -expm1(x_c - lse) with lse the fp32 row scratch,
    and the rounding of lse (an ulp is 2^-20 between 8 and 16) reaches r_c = p_c / (1 - p_c) multiplied by p_c / (1 - p_c)^2: a context
    word the model is all but sure of (1 - p_c ~ 1e-3, which an 8-word vocabulary with a +6 lift draws readily) carries an error of 1e-3
    relative in its gradient entry whatever a kernel does with fp32 sums, while the bound is 5e-6 of the largest entry.  The draws are
    judged by the float64 reference alone.  The clamp has a test of its own below."""
    for k in range(40):
        c = draw_case(N, T, V, W, 700 + N + T + W + 100 * k)
        if c["mean_ul"] >= MIN_MEAN_UL and c["condition"] <= MAX_CONDITION:
            return c
    raise AssertionError("no regular case among 40 draws for %r" % ((N, T, V, W),))


@functools.lru_cache(maxsize=None)
def reference(shape, weights):
    c = case(*shape)
    cw, fw, gamma, ua, smoothing = weights
    ref = R.token_loss(c["z"], c["y"], c["cand"], smoothing, cw, fw, gamma, ua, 1.7 * c["P"])
    _, ref["w"], ref["R"] = R.closed_form_grad(c["z"], c["y"], c["cand"], smoothing, cw, fw, gamma, ua)
    return ref


def run_kernels(z, y, weights, caps=None, src=None, g=1.0, misalign=False, pad=PAD, backward=True):
    """sat_token_loss_fwd / _bwd through the C ABI, every output inside a guard band.  ``misalign`` moves logits and dlogits one float
    off their 16-byte alignment (the 4-byte form).  ``caps`` / ``src`` None: NULL context and src_row."""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    P, V = z.shape
    cw, fw, gamma, ua, smoothing = weights
    off = 1 if misalign else 0
    buf = torch.empty(P * V + 4, dtype=torch.float32, device="cuda")
    zd = buf[off:off + P * V].view(P, V)
    zd.copy_(z)
    assert (zd.data_ptr() % 16 != 0) == misalign
    yd = y.to(torch.int32).cuda()
    cd = None if caps is None else caps.to(torch.int32).cuda().contiguous()
    sd = None if src is None else src.to(torch.int32).cuda().contiguous()
    N, T = (0, 0) if caps is None else caps.shape
    gd = torch.tensor([g], dtype=torch.float32, device="cuda")
    o = dict(dlogits=Banded(P * V, off=off), out=Banded(6), lse=Banded(P), aux=Banded(2 * P), rows=Banded(4 * P), correct=Banded(P, torch.int32))
    head = (L.ptr(zd), L.ptr(yd), P, V, smoothing, cw, fw, gamma, ua, L.ptr(cd), L.ptr(sd), N, T, pad)
    L.check(lib.sat_token_loss_fwd(*head, L.ptr(o["lse"].view), L.ptr(o["aux"].view), L.ptr(o["rows"].view), L.ptr(o["correct"].view), L.ptr(o["out"].view),
                                   L.stream_ptr()), "sat_token_loss_fwd")
    if backward:
        L.check(lib.sat_token_loss_bwd(*head, L.ptr(o["lse"].view), L.ptr(o["aux"].view), L.ptr(gd), L.ptr(o["dlogits"].view), L.stream_ptr()), "sat_token_loss_bwd")
    torch.cuda.synchronize()
    got = dict(out=o["out"].view.cpu(), lse=o["lse"].view.cpu(), aux=o["aux"].view.cpu().view(P, 2), rows=o["rows"].view.cpu().view(P, 4),
               correct=o["correct"].view.cpu(), grad=o["dlogits"].view.cpu().view(P, V))
    got["intact"] = all(b.intact() for b in o.values())
    return got


def check_against_reference(ref, got, weights, what):
    cw, fw, gamma, ua, smoothing = weights
    assert got["intact"], what + ": a guard band was written"
    close(got["lse"], ref["lse"], what=what + " lse")
    for j, name in enumerate(("ce", "fl", "ul", "mass")):
        close(got["rows"][:, j], ref["rows"][:, j], what=what + " %s rows" % name)
    if fw != 0:
        close(got["aux"][:, 0], ref["w"], what=what + " w rows")
    if ua != 0:
        close(got["aux"][:, 1], ref["R"], what=what + " R rows")
    P = ref["rows"].shape[0]
    mags = [float(ref["rows"][:, j].abs().sum()) / P for j in range(4)]
    for i, name, terms in ((0, "loss", cw * mags[0] + fw * mags[1] + ua * mags[2]), (2, "ce", mags[0]), (3, "fl", mags[1]), (4, "ul", mags[2]),
                           (5, "mass", mags[3])):
        err = abs(float(got["out"][i]) - float(ref[name]))
        print("%s mean %s: |d|=%.3e (sum of |terms| %.3g)" % (what, name, err, terms))
        assert err <= TOL * max(1.0, terms), (what, name, float(got["out"][i]), float(ref[name]))
    assert float(got["out"][1]) == float(np.float32(float(ref["accuracy"]))), what + ": accuracy"
    close(got["grad"], ref["grad"], what=what + " dlogits")


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_token_loss_kernels_against_the_reference(shape, weights):
    c, ref = case(*shape), reference(shape, weights)
    what = "N=%d T=%d V=%d W=%d weights=%s" % (*shape, weights)
    n_cand = [len(x) for x in c["cand"]]
    print("%s: P=%d, %d non-empty rows, at most %d candidates, reference mean ul %.4g, min (1 - p_c) %.4g" %
          (what, c["P"], sum(n > 0 for n in n_cand), max(n_cand), float(ref["ul"]), ref["min_one_minus_p"]))
    if weights[3] != 0:                          # the case exercises the term, away from the clamp
        assert float(ref["ul"]) >= MIN_MEAN_UL and ref["min_one_minus_p"] >= 1e-3 and c["condition"] <= MAX_CONDITION
    if shape[3] == 40:
        assert max(n_cand) > 20
    got = run_kernels(c["z"], c["y"], weights, c["caps"], c["src"], 1.7 * c["P"])
    check_against_reference(ref, got, weights, what)


def test_one_float_of_misalignment_takes_the_4_byte_form():
    shape, weights = SHAPES[3], WEIGHTS[3]
    assert shape[2] % 4 == 0
    c, ref = case(*shape), reference(shape, weights)
    got = run_kernels(c["z"], c["y"], weights, c["caps"], c["src"], 1.7 * c["P"])
    mis = run_kernels(c["z"], c["y"], weights, c["caps"], c["src"], 1.7 * c["P"], misalign=True)
    check_against_reference(ref, mis, weights, "misaligned")
    close(mis["grad"], got["grad"], what="misaligned against aligned dlogits")
    close(mis["out"], got["out"], what="misaligned against aligned out")
    assert torch.equal(mis["correct"], got["correct"])


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[6]])
def test_two_runs_give_the_same_bits(shape):
    c, weights = case(*shape), WEIGHTS[3]
    a = run_kernels(c["z"], c["y"], weights, c["caps"], c["src"], 1.7 * c["P"])
    junk = torch.full((1 << 24,), float("nan"), device="cuda"); del junk           # recycled blocks now hold NaN
    b = run_kernels(c["z"], c["y"], weights, c["caps"], c["src"], 1.7 * c["P"])
    assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("out", "lse", "aux", "rows", "correct", "grad"))


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]])
def test_the_cross_entropy_alone_is_the_label_smoothing_kernels_bit_for_bit(shape, misalign):
    """weights (1, 0, ., 0): out[0..1], lse_rows and dlogits of sat_ce_label_smooth_fwd / _bwd; context and src_row are NULL"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    c = case(*shape)
    P, V = c["z"].shape
    for smoothing in (0.0, 0.1):
        got = run_kernels(c["z"], c["y"], (1.0, 0.0, 2.0, 0.0, smoothing), None, None, 1.7 * P, misalign)
        assert got["intact"]
        off = 1 if misalign else 0
        buf = torch.empty(P * V + 4, dtype=torch.float32, device="cuda")
        zd = buf[off:off + P * V].view(P, V); zd.copy_(c["z"])
        yd = c["y"].to(torch.int32).cuda()
        gd = torch.tensor([1.7 * P], dtype=torch.float32, device="cuda")
        dl = Banded(P * V, off=off)
        lse, rws, out = torch.empty(P, device="cuda"), torch.empty(P, device="cuda"), torch.empty(2, device="cuda")
        correct = torch.empty(P, dtype=torch.int32, device="cuda")
        L.check(lib.sat_ce_label_smooth_fwd(L.ptr(zd), L.ptr(yd), P, V, smoothing, L.ptr(lse), L.ptr(rws), L.ptr(correct), L.ptr(out), L.stream_ptr()), "ce fwd")
        L.check(lib.sat_ce_label_smooth_bwd(L.ptr(zd), L.ptr(yd), L.ptr(lse), P, V, smoothing, L.ptr(gd), L.ptr(dl.view), L.stream_ptr()), "ce bwd")
        torch.cuda.synchronize()
        for name, a, b in (("out[0..1]", got["out"][:2], out.cpu()), ("lse", got["lse"], lse.cpu()), ("ce rows", got["rows"][:, 0], rws.cpu()),
                           ("dlogits", got["grad"], dl.view.cpu().view(P, V))):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, smoothing, float((a.double() - b.double()).abs().max()))
        assert torch.equal(got["correct"], correct.cpu()) and float(got["out"][2]) == float(out[0])
        assert bool((got["out"][3:] == 0).all()) and bool((got["rows"][:, 1:] == 0).all())


def test_a_null_context_serves_when_ul_alpha_is_zero():
    shape, weights = SHAPES[2], WEIGHTS[1]
    c, ref = case(*shape), reference(shape, weights)
    check_against_reference(ref, run_kernels(c["z"], c["y"], weights, None, None, 1.7 * c["P"]), weights, "NULL context")


def test_a_target_outside_the_vocabulary_gives_a_nan_row_and_no_stray_access():
    shape = SHAPES[2]
    c = case(*shape)
    V = shape[2]
    for bad in (V, -1):
        yb = c["y"].clone(); yb[2] = bad
        others = [p for p in range(c["P"]) if p != 2]
        for weights in (WEIGHTS[0], WEIGHTS[1]):
            for misalign in (False, True):
                got = run_kernels(c["z"], yb, weights, c["caps"], c["src"], 1.7 * c["P"], misalign)
                assert got["intact"], (bad, weights, misalign)
                col = 0 if weights[0] != 0 else 1
                assert bool(torch.isnan(got["rows"][2, col])) and bool(torch.isnan(got["out"][0])) and bool(torch.isnan(got["out"][2 + col]))
                assert bool(torch.isfinite(got["rows"][others]).all()) and bool(torch.isfinite(got["grad"][others]).all()) and int(got["correct"][2]) == 0
    sb = c["src"].clone(); sb[3] = (shape[1] - 1) * shape[0]                      # a source row outside the captions: a NaN ul row, nothing read
    got = run_kernels(c["z"], c["y"], WEIGHTS[0], c["caps"], sb, 1.7 * c["P"])
    assert got["intact"] and bool(torch.isnan(got["rows"][3, 2])) and bool(torch.isfinite(got["rows"][[0, 1, 2, 4]]).all())


@pytest.mark.parametrize("V", [1003, 4100])
def test_a_candidate_on_the_clamp_adds_the_clamps_log_and_passes_no_gradient(V):
    """one context id at logit +40: 1 - p_c is 0 in fp32, below the clamp of 1e-5"""
    N, T, ua, P = 1, 5, 0.5, 4
    caps = torch.tensor([[V - 2, 7, 9, 11, V - 1]])
    src = torch.arange(4, dtype=torch.int32)                                     # one caption: row t is step t
    y = caps[0, 1:]
    z = rows(P, V, 1, 900 + V)[0]
    z[2, 7] = 40.0                                                               # row 2: context {7, 9}, target 11
    weights = (1.0, 1.0, 2.0, ua, 0.1)
    cand = [[], [7], [7, 9], [7, 9, 11]]
    ref = R.token_loss(z, y, cand, 0.1, 1.0, 1.0, 2.0, ua, 1.7 * P)
    _, ref["w"], ref["R"] = R.closed_form_grad(z, y, cand, 0.1, 1.0, 1.0, 2.0, ua)
    got = run_kernels(z, y, weights, caps, src, 1.7 * P)
    assert got["intact"] and all(bool(torch.isfinite(got[k]).all()) for k in ("out", "lse", "aux", "rows", "grad"))
    p9 = float(torch.softmax(z[2].double(), 0)[9])
    want = -float(np.log(1e-5)) - float(np.log1p(-p9))
    print("ul row on the clamp: %.7f, want %.7f" % (float(got["rows"][2, 2]), want))
    assert abs(float(got["rows"][2, 2]) - want) <= TOL * want
    R_p = float(got["aux"][2, 1])
    assert abs(R_p - p9 / (1.0 - p9)) <= TOL                                      # candidate 7 adds no r_c
    # the clamped candidate's entry: the dense part alone, (ce_weight + focal_weight w - ul_alpha R) p_c - ce_weight smoothing / V
    w_p = float(got["aux"][2, 0])
    dense = 1.7 * ((1.0 + w_p - ua * R_p) * 1.0 - 0.1 / V)
    print("gradient at the clamped candidate: %.7f, want %.7f" % (float(got["grad"][2, 7]), dense))
    assert abs(float(got["grad"][2, 7]) - dense) <= TOL * max(1.0, abs(dense))
    only = run_kernels(z, y, (0.0, 0.0, 2.0, ua, 0.0), caps, src, 1.7 * P)        # the unlikelihood alone: exactly -ul_alpha p_c R_p gscale / P
    assert abs(float(only["grad"][2, 7]) - (-ua * 1.0 * float(only["aux"][2, 1]) * 1.7)) <= TOL
    check_against_reference(ref, got, weights, "clamp row V=%d" % V)


def test_a_certain_target_has_a_finite_focal_gradient():
    """q == 1 in fp32 at gamma = 0.5, where (1 - q)^(gamma - 1) is infinite"""
    P, V = 3, 1003
    z = rows(P, V, 1, 950)[0]
    y = torch.tensor([5, 17, 400])
    z[1, 17] = 60.0
    for weights in ((0.0, 1.0, 0.5, 0.0, 0.0), (1.0, 1.0, 0.5, 0.0, 0.1)):
        got = run_kernels(z, y, weights, None, None, 1.7 * P)
        assert got["intact"] and all(bool(torch.isfinite(got[k]).all()) for k in ("out", "lse", "aux", "rows", "grad"))
        assert float(got["rows"][1, 1]) == 0.0 and float(got["aux"][1, 0]) == 0.0
        ref = R.token_loss(z, y, [[]] * P, weights[4], weights[0], weights[1], 0.5, 0.0, 1.7 * P)
        close(got["grad"][[0, 2]], ref["grad"][[0, 2]], what="the other rows")


def test_token_loss_fn_returns_the_reference():
    import sat_amd  # noqa: F401
    from sat_amd import decoder as Dk
    shape, weights = SHAPES[3], WEIGHTS[3]
    c, ref = case(*shape), reference(shape, weights)
    cw, fw, gamma, ua, smoothing = weights
    zd = c["z"].cuda().requires_grad_()
    loss, acc, terms = Dk.TokenLossFn.apply(zd, c["y"].to(torch.int32).cuda(), smoothing, cw, fw, gamma, ua, c["caps"].to(torch.int32).cuda(), c["src"].cuda(), PAD)
    assert loss.requires_grad and not acc.requires_grad and not terms.requires_grad and tuple(terms.shape) == (4,)
    (loss * (1.7 * c["P"])).backward()
    close(loss, ref["loss"], what="loss"); close(zd.grad, ref["grad"], what="gradient")
    close(terms, torch.stack([ref["ce"], ref["fl"], ref["ul"], ref["mass"]]), what="terms")
    with pytest.raises(ValueError, match="ul_alpha"):
        Dk.TokenLossFn.apply(zd, c["y"].to(torch.int32).cuda(), smoothing, cw, fw, gamma, ua, None, None, PAD)


# ---------------------------------------------------------------------------------------------------------------- the whole step
def step_batch(hp):
    """test_gpu_train_step.py's batch (B = 6, R = 3, T = 9) with the caption words remapped into 1..5, so that contexts repeat"""
    from test_gpu_train_step import batch
    img, caps, lengths = batch(hp)
    word = (caps > 0) & (caps < hp.vocab_size - 2)
    return img, torch.where(word, 1 + (caps - 1) % 5, caps), lengths


def _step(model, b):
    img, caps, lengths = b
    out = model.training_step((img.cuda(), caps.cuda(), lengths), 0)
    out["loss"].backward()
    torch.cuda.synchronize()
    return out


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


KEYS = {"loss", "accuracy", "epsilon_tf", "ce", "fl", "ul", "repeat_mass"}
FULL = dict(token_loss="ce+fl", focal_gamma=2.0, ul_alpha=1.0, label_smoothing=0.1)


@pytest.mark.parametrize("eps,layers,over", [(1.0, 1, FULL), (0.0, 1, FULL), (1.0, 2, dict(ul_alpha=1.0))])
def test_token_loss_training_step_matches_oracle(eps, layers, over):
    from test_gpu_train_step import make, rel
    model, oracle, hp = make(dict(over, decoder_tf="always" if eps == 1.0 else None, decoder_layers=layers))
    img, caps, lengths = step_batch(hp)
    ann = oracle.encoder(img.clone())
    loss_o, out_o = R.training_loss_token(oracle.sd, oracle.hp, ann, caps, lengths, over.get("token_loss", "ce"), over.get("focal_gamma", 2.0),
                                          over["ul_alpha"], eps, pad_id=model.pad_idx)
    loss_o.backward()
    assert max(len(c) for c in out_o["candidates"]) >= 2
    metrics = _step(model, (img, caps, lengths))
    assert set(metrics) == KEYS
    for k in ("ce", "fl", "ul", "repeat_mass"):
        got, ref = float(metrics[k]), float(out_o[k])
        print("%s: hip %.9g oracle %.9g" % (k, got, ref))
        assert metrics[k].is_cuda and not metrics[k].requires_grad
        assert abs(got - ref) <= 1e-5 * abs(ref), (k, got, ref)
    assert float(out_o["ul"]) > 0 and (float(out_o["fl"]) > 0) == ("token_loss" in over)
    print("loss: hip %.9g oracle %.9g (without the terms %.9g)" % (metrics["loss"].item(), loss_o.item(), float(out_o["base"])))
    assert abs(metrics["loss"].item() - loss_o.item()) <= 1e-4 * max(1.0, abs(loss_o.item()))
    assert abs(float(metrics["accuracy"]) - float(out_o["acc"])) < 1e-6
    assert abs(loss_o.item() - float(out_o["base"])) > 1e-3                       # the terms are in the loss
    og = oracle.named_grads()
    worst = (0.0, None)
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        e = float((p.grad.cpu().double() - og[k].double()).norm()) / max(1e-9, float(og[k].double().norm()))
        worst = max(worst, (e, k))
        assert e <= 2e-2, "%s: relative L2 gradient error %.3e" % (k, e)
    print("worst relative L2 gradient error: %.3e (%s)" % worst)
    for k in ("attention.f_att.weight", "output.output.weight", "lstm.weight_hh_l0", "embedding.weight", "encoder.9.weight"):
        p = dict(model.named_parameters())[k]
        print("%s: %.3e" % (k, rel(p.grad, og[k])))
        assert rel(p.grad, og[k]) <= 5e-4, k


def test_default_hyper_parameters_are_the_plain_step():
    from test_gpu_train_step import make
    got = []
    for over in (dict(token_loss="ce", ul_alpha=0), {}):
        model, _, hp = make(dict(over, decoder_tf="always", label_smoothing=0.1))
        metrics = _step(model, step_batch(hp))
        assert set(metrics) == {"loss", "accuracy", "epsilon_tf"}
        got.append((metrics["loss"].detach().clone(), _grads(model)))
    (la, ga), (lb, gb) = got
    assert torch.equal(la, lb) and ga.keys() == gb.keys()
    assert [k for k in ga if not torch.equal(ga[k], gb[k])] == []


def test_token_loss_composes_with_the_activation_regularisers():
    from test_gpu_train_step import make
    model, _, hp = make(dict(FULL, decoder_tf="always", ar_alpha=2.0, tar_beta=1.0))
    metrics = _step(model, step_batch(hp))
    assert set(metrics) == KEYS | {"ar", "tar"} and all(bool(torch.isfinite(torch.as_tensor(v))) for v in metrics.values())
    plain, _, _ = make(dict(FULL, decoder_tf="always"))
    base = _step(plain, step_batch(hp))
    want = float(base["loss"].detach()) + 2.0 * float(metrics["ar"]) + 1.0 * float(metrics["tar"])
    assert abs(float(metrics["loss"].detach()) - want) <= 1e-5 * abs(want) and torch.equal(metrics["ul"], base["ul"])


def test_bf16_mode_is_finite_and_reproducible():
    """the logits come out of bf16 MFMA products in bf16 mode: the deviation of the terms from fp32 mode is printed, not asserted"""
    from test_gpu_train_step import make
    got = []
    for mode in ("bf16", "bf16", "fp32"):
        model, _, hp = make(dict(FULL, decoder_tf="always"))
        model.set_precision(mode)
        m = _step(model, step_batch(hp))
        got.append(({k: m[k].detach().clone() for k in ("loss", "ce", "fl", "ul", "repeat_mass")}, _grads(model)))
    (ma, ga), (mb, gb), (mf, _) = got
    assert all(bool(torch.isfinite(v)) for v in ma.values()) and all(bool(torch.isfinite(v).all()) for v in ga.values())
    assert all(torch.equal(ma[k], mb[k]) for k in ma) and [k for k in ga if not torch.equal(ga[k], gb[k])] == []
    for k in ma:
        print("bf16 mode %s: %.9g  fp32 mode: %.9g  relative deviation %.3e" % (k, float(ma[k]), float(mf[k]), abs(float(ma[k]) - float(mf[k])) / abs(float(mf[k]))))


def test_graph_replay_equals_the_eager_token_loss_step():
    from sat_amd.graph import GraphedTrainStep
    from test_gpu_graph import _batch, _make, _same, _state
    eager, hp = _make("fp32", FULL)
    graphed, _ = _make("fp32", FULL)
    opt_e, opt_g = eager.configure_optimizers(), graphed.configure_optimizers()
    step = GraphedTrainStep(graphed, opt_g)
    img, caps, lengths = _batch(hp, 11)
    word = (caps > 0) & (caps < hp.vocab_size - 2)
    b = (img, torch.where(word, 1 + (caps - 1) % 5, caps), lengths)
    for it in range(4):          # step 0 warms eagerly, step 1 captures and replays, steps 2 and 3 replay
        opt_e.zero_grad(set_to_none=True)
        out_e = eager.training_step(b, it)
        out_e["loss"].backward()
        opt_e.step()
        out_g = step(b, it)
        assert set(out_g) == KEYS
        for k in ("loss", "ce", "fl", "ul", "repeat_mass"):
            assert torch.equal(out_e[k].detach(), out_g[k]), "step %d: %s %r vs %r" % (it, k, float(out_e[k]), float(out_g[k]))
        _same(_state(eager, opt_e), _state(graphed, opt_g), "after step %d" % it)
    assert float(out_g["ul"]) > 0 and float(out_g["fl"]) > 0
    assert step.stats["captured"] == 1 and step.stats["replayed"] == 3, dict(step.stats)
    assert [k for k in step.stats if k.startswith("eager")] == ["eager: first step of a shape / plan"], dict(step.stats)
