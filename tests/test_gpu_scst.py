"""GPU: self-critical sequence training ("Self-critical training") against its float64 specification (tests/scst_ref.py) and
the CPU oracle: the policy-loss kernels (csrc/policy_loss.hip), sat_scst_prepare, ancestral sampling in the batched search
(SAT_SAMPLE_ANCESTRAL) and the whole step (sat_amd/scst.py, SAT.scst_step).

Tolerances.  The policy kernels: 5e-6 of the largest reference entry (floored at 1), the bound test_label_smoothing_kernel_vector_and_
scalar_paths holds the same arithmetic to; the weights and scales used here make the largest gradient entry O(1), so the floor does not
hide it.  The loss, a signed sum, is held to the same 5e-6 of the sum of the magnitudes of its terms.  sat_scst_prepare: integers and masks
exactly, floats within 1e-6 relative (one fp32 rounding of an fp64 result is 6e-8).  The ancestral search: exact words, under the asserted
precondition that no compared top-two key gap of the oracle is below 1e-3, ten times the project's 1e-4 fp32 bound on scores.  The whole
step: test_gpu_train_step.py's loss bound 1e-4 max(1, |loss|) and 1e-3 relative norm for every parameter gradient (on the damped net).  Rewards: CIDEr-D and
ROUGE-L as test_gpu_consensus.py holds them (1e-9, 1e-12) plus the fp32 rounding of the float the step reports (2^-24 relative)."""
import ctypes as C

import numpy as np
import pytest
import torch

import scst_ref as R

pytestmark = pytest.mark.gpu

TOL = 5e-6
CIDER_TOL, ROUGE_TOL = 1e-9, 1e-12
GUMBEL_SEED, SEARCH_T = 4, 0.8        # chosen on the CPU with the oracle alone (test_ancestral_search_draws_the_oracles_words)


def ids_for(V):
    """(START, PAD, END, UNK) where oracle.default_hparams puts them"""
    return (V - 2, 0, V - 1, V - 3)


def rows(P, V, seed):
    """logits ~ 3 N(0, 1)-like (uniform sums), targets among the never-masked ids, weights of both signs with one zero"""
    from oracle import prng
    x = (prng.uniform((P, V), seed, -1.0, 1.0) + prng.uniform((P, V), seed + 1, -1.0, 1.0) + prng.uniform((P, V), seed + 2, -1.0, 1.0)) * 3.0
    t = prng.integers((P,), seed + 3, 1, V - 3)
    w = prng.uniform((P,), seed + 4, -2.0, 2.0)
    w[P // 2] = 0.0
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(t), torch.from_numpy(w.astype(np.float32))


def close(a, b, tol=TOL, what=""):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print("%s: max|d|=%.3e (scale %.3g, tol %.1e)" % (what, err, scale, tol))
    assert err <= tol * scale, "%s: max|d|=%.3e (scale %.3g, tol %.1e)" % (what, err, scale, tol)


BAND = 64            # floats of NaN on either side of dlogits


def run_kernels(x, t, w, inv_t, ids, n_first, scale, g, misalign=False):
    """sat_policy_nll_fwd / _bwd through the C ABI.  dlogits lies inside a NaN guard band and starts as NaN; ``misalign`` moves logits and
    dlogits one float off their 16-byte alignment (the 4-byte form).  Returns (loss, logq, lse, dlogits, the whole band buffer)."""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    P, V = x.shape
    off = 1 if misalign else 0
    xbuf = torch.empty(P * V + 4, dtype=torch.float32, device="cuda")
    xv = xbuf[off:off + P * V].view(P, V)
    xv.copy_(x)
    assert (xv.data_ptr() % 16 != 0) == misalign
    buf = torch.full((P * V + 2 * BAND + 4,), float("nan"), dtype=torch.float32, device="cuda")
    dl = buf[BAND + off:BAND + off + P * V].view(P, V)
    td, wd = t.to(torch.int32).cuda(), w.cuda()
    idd = torch.tensor(ids, dtype=torch.int32, device="cuda")
    gd = torch.tensor([g], dtype=torch.float32, device="cuda")
    lse, logq, out = (torch.empty(P, device="cuda"), torch.empty(P, device="cuda"), torch.empty(1, device="cuda"))
    L.check(lib.sat_policy_nll_fwd(L.ptr(xv), L.ptr(td), L.ptr(wd), P, V, inv_t, L.ptr(idd), n_first, scale, L.ptr(lse), L.ptr(logq), L.ptr(out),
                                   L.stream_ptr()), "sat_policy_nll_fwd")
    L.check(lib.sat_policy_nll_bwd(L.ptr(xv), L.ptr(td), L.ptr(wd), L.ptr(lse), P, V, inv_t, L.ptr(idd), n_first, scale, L.ptr(gd), L.ptr(dl),
                                   L.stream_ptr()), "sat_policy_nll_bwd")
    torch.cuda.synchronize()
    return out.cpu(), logq.cpu(), lse.cpu(), dl.cpu(), (buf.cpu(), BAND + off, P * V)


def check_against_reference(x, t, w, inv_t, ids, n_first, scale, g, got, what):
    loss, logq, lse, dl, (buf, lo, n) = got
    P, V = x.shape
    xd = x.double()
    ref_loss, ref_logq, ref_lse = R.policy_loss(xd, t, w.double(), inv_t, ids, n_first, scale)
    ref_grad = R.policy_grad(xd, t, w.double(), inv_t, ids, n_first, scale, g)
    close(lse, ref_lse, what=what + " lse"); close(logq, ref_logq, what=what + " logq")
    terms = float((scale * w.double() * ref_logq).abs().sum())
    err = abs(float(loss) - float(ref_loss))
    print("%s loss: |d|=%.3e (sum of |terms| %.3g)" % (what, err, terms))
    assert err <= TOL * max(1.0, terms), (what, float(loss), float(ref_loss))
    close(dl, ref_grad, what=what + " dlogits")
    keep = R.unmasked(P, V, ids, n_first)
    assert bool((dl[~keep] == 0).all()), what + ": a masked column is not exactly 0"
    assert bool((dl[w == 0] == 0).all()), what + ": a row of weight zero is not exactly 0"
    assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all()), what + ": the guard band was written"


@pytest.mark.parametrize("P,V", [(7, 10000), (5, 1003), (3, 8), (9, 4100), (2, 7)])
def test_policy_kernels_against_the_reference(P, V):
    x, t, w = rows(P, V, 100 + P)
    ids = ids_for(V)
    for inv_t in (1.0, 1 / 0.7):
        for n_first in (0, 2, P):
            got = run_kernels(x, t, w, inv_t, ids, n_first, 1.0, 1.7)
            check_against_reference(x, t, w, inv_t, ids, n_first, 1.0, 1.7, got, "P=%d V=%d 1/T=%.3f first=%d" % (P, V, inv_t, n_first))
    again = run_kernels(x, t, w, 1 / 0.7, ids, 2, 1.0, 1.7)                       # two runs, the same bits
    for a, b in zip(run_kernels(x, t, w, 1 / 0.7, ids, 2, 1.0, 1.7)[:4], again[:4]):
        assert torch.equal(a, b)
    got = run_kernels(x, t, w, 1 / 0.7, ids, 2, 0.25, 1.0, misalign=True)         # one float off the alignment: the 4-byte form
    check_against_reference(x, t, w, 1 / 0.7, ids, 2, 0.25, 1.0, got, "P=%d V=%d misaligned" % (P, V))
    zero = torch.zeros(P)
    loss, logq, _, dl, (buf, lo, n) = run_kernels(x, t, zero, 1.0, ids, P, 1.0, 1.0)
    assert float(loss) == 0.0 and bool((dl == 0).all()) and bool(torch.isfinite(logq).all())      # a zero-only batch
    assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all())


@pytest.mark.parametrize("P,V", [(7, 10000), (5, 1003)])
def test_policy_loss_is_cross_entropy_when_nothing_is_masked_away(P, V):
    """all weights 1, scale 1 / P, no first rows, the two masked columns at -1e30: LabelSmoothing(0.0) on the same logits"""
    import sat_amd  # noqa: F401
    from sat_amd import decoder as Dk, model as M
    x, t, _ = rows(P, V, 300 + P)
    ids = ids_for(V)
    x[:, ids[0]] = -1e30; x[:, ids[1]] = -1e30
    xa, xb = x.cuda().requires_grad_(), x.cuda().requires_grad_()
    ce = M.LabelSmoothing(0.0)(xa, t.cuda()); (ce * 1.7).backward()
    pl = Dk.PolicyNLLFn.apply(xb, t.to(torch.int32).cuda(), torch.ones(P, device="cuda"), 1.0, torch.tensor(ids, dtype=torch.int32, device="cuda"), 0,
                              1.0 / P)
    (pl * 1.7).backward()
    close(pl, ce, what="loss"); close(xb.grad, xa.grad, what="gradient")
    assert bool((xb.grad[:, [ids[0], ids[1]]] == 0).all())


def test_policy_loss_bad_targets_give_nan_and_no_fault():
    P, V = 6, 1003
    x, t, w = rows(P, V, 77)
    w[P // 2] = 0.5
    ids = ids_for(V)
    for bad, n_first in ((-1, 0), (V, 0), (V + 1000000, 0), (-2 ** 31, 0), (ids[0], 0), (ids[1], P), (ids[2], 3), (ids[3], P)):
        tb = t.clone(); tb[2] = bad
        loss, logq, lse, dl, (buf, lo, n) = run_kernels(x, tb, w, 1.0, ids, n_first, 1.0, 1.0)
        assert bool(torch.isnan(loss).all()) and bool(torch.isnan(logq[2])), (bad, n_first)
        assert bool(torch.isfinite(logq[[0, 1, 3, 4, 5]]).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(dl).all())
        assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all())
    tb = t.clone(); tb[4] = ids[2]                                                # END is a legal target after the first step
    assert bool(torch.isfinite(run_kernels(x, tb, w, 1.0, ids, 3, 1.0, 1.0)[0]).all())


# ---------------------------------------------------------------------------------------------------------------- sat_scst_prepare
@pytest.mark.parametrize("baseline", ["mean", "greedy"])
def test_prepare_against_the_reference(baseline):
    import sat_amd  # noqa: F401
    from sat_amd import scst
    from oracle import prng
    B, K, S = 2, 3, 5
    ids = ids_for(60)
    for lens in ([1, 2, S - 1, S, 3, S], [0, 2, S + 3, S, 1, S - 1]):             # the second: a length of 0 and one of S + 3 are clamped
        tok = prng.integers((B * K, S + 1), 9, 1, 57).astype(np.int32)
        ln = np.array(lens, np.int32)
        sc = prng.uniform((B * K, 2), 21, 0.0, 3.0).astype(np.float64)
        sg = prng.uniform((B, 2), 22, 0.0, 3.0).astype(np.float64)
        want = R.prepare(tok, ln, sc, sg, K, 1.0, 0.5, R.GREEDY if baseline == "greedy" else R.MEAN, ids)
        got = scst.prepare(torch.from_numpy(tok).cuda(), torch.from_numpy(ln).cuda(), torch.from_numpy(sc).cuda(), K, ids, baseline, (1.0, 0.5),
                           torch.from_numpy(sg).cuda() if baseline == "greedy" else None)
        torch.cuda.synchronize()
        for k in ("caps", "lengths", "count"):
            assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), want[k]), (k, lens)
        assert np.array_equal(got["step_weight"].cpu().numpy() != 0, want["step_weight"] != 0) and bool((want["advantage"] != 0).all())
        for k in ("reward", "baseline", "advantage", "step_weight"):
            g, w_ = got[k].cpu().numpy().astype(np.float64), want[k].astype(np.float64)
            assert np.all(np.abs(g - w_) <= 1e-6 * np.abs(w_)), (k, lens, g, w_)


# ---------------------------------------------------------------------------------------------------------------- the search
OVER = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16,
            decoder_dim=40, deep_output=True, val_beamk=3, val_max_len=7)


def tiny(device="cuda", damp_residual=None):
    """the tiny model of test_gpu_consensus.py::_val_model (same hyper-parameters, same seed) and the oracle on its weights.
    ``damp_residual``: the last BatchNorm weight of every residual branch, as test_gpu_train_step.py::make and test_gpu_encoder.py::_damp
    set it for the well-conditioned variant of the net (a freshly initialised ResNet doubles its activation scale every block, and a
    pre-activation within fp32 rounding of zero then takes the other side of a ReLU in one of two correct fp32 evaluations)."""
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    torch.manual_seed(5)
    model = M.SAT(**vars(O.default_hparams(**OVER)))
    if damp_residual is not None:
        with torch.no_grad():
            for blk in [b for li in (5, 6, 7, 8) for b in model.encoder[li]]:
                (blk.bn3 if blk.kind == "bottleneck" else blk.bn2).weight.fill_(damp_residual)
    oracle = O.OracleSAT(O.default_hparams(**OVER), {k: v.detach().clone() for k, v in model.state_dict().items()})
    return model.to(device), oracle


def batch(seed, B=4):
    from oracle import prng
    img = torch.from_numpy(prng.uniform((B, 3, 64, 64), seed, 0.0, 1.0))
    caps, lengths = prng.captions(B, 3, 9, 60, seed + 1, min_len=3)
    return img, torch.from_numpy(caps), torch.from_numpy(lengths)


def ancestral_case(oracle, seed=GUMBEL_SEED, B=3, K=4, S=6):
    """annotations of B images from the oracle's encoder in eval mode (both sides search the same numbers) and a Gumbel table
    (S + 1, B * K, V) from prng"""
    from oracle import prng
    img = torch.from_numpy(prng.uniform((B, 3, 64, 64), 31, 0.0, 1.0))
    oracle.encoder.eval()
    with torch.no_grad():
        ann_img = oracle.encoder(img.clone())                                    # (B, D, h, w)
    oracle.encoder.train()
    u = prng.uniform((S + 1, B * K, 60), seed, 1e-6, 1.0 - 1e-6).astype(np.float64)
    gumbel = torch.from_numpy((-np.log(-np.log(u))).astype(np.float32))
    return ann_img, gumbel


def oracle_replay(oracle, ann_img, tokens, lengths, gumbel, K, S, temperature):
    """Teacher-force the captions through the oracle and redo every draw: (words the oracle draws at the compared steps, the captions'
    words there, the smallest top-two key gap).  Row n, step t < len drew word t + 1; step len < S drew END; a cut caption (len == S)
    is compared on its S draws."""
    from oracle import sat_oracle as O
    hp = oracle.hp
    N = tokens.shape[0]
    B = N // K
    ids = ids_for(hp.vocab_size)
    T = S + 2
    caps = torch.zeros(N, T, dtype=torch.int64)
    caps[:, 0] = ids[0]
    for n in range(N):
        ln = int(lengths[n])
        caps[n, 1:1 + ln] = tokens[n, :ln].long()
        caps[n, 1 + ln] = ids[2]
    lens = (lengths.long() + 1).clamp(max=S + 1)
    with torch.no_grad():
        sd = {k: v.detach() for k, v in oracle.sd.items()}
        out = O.decode_train(sd, hp, ann_img, caps.reshape(B, K, T), lens.reshape(B, K), epsilon=1.0)
    drawn, wanted, gap = [], [], float("inf")
    for n in range(N):
        ln = int(lengths[n])
        for t in range(ln + 1 if ln < S else S):
            word, g = R.ancestral_draw(out["logits"][n, t].double(), temperature, ids if t == 0 else ids[:2], gumbel[t, n].double())
            drawn.append(word); wanted.append(int(caps[n, t + 1])); gap = min(gap, g)
    return drawn, wanted, gap


def test_ancestral_search_draws_the_oracles_words():
    import sat_amd  # noqa: F401
    from sat_amd import scst
    model, oracle = tiny()
    B, K, S = 3, 4, 6
    ann_img, gumbel = ancestral_case(oracle)
    ann = ann_img.permute(0, 2, 3, 1).reshape(B, -1, ann_img.shape[1]).contiguous().cuda()
    tokens, lengths = scst.sample(model, ann, K, S, SEARCH_T, gumbel=gumbel.cuda())
    again = scst.sample(model, ann, K, S, SEARCH_T, gumbel=gumbel.cuda())
    assert torch.equal(tokens, again[0]) and torch.equal(lengths, again[1])
    tokens, lengths = tokens.cpu(), lengths.cpu()
    assert tuple(tokens.shape) == (B * K, S + 1) and int(lengths.min()) >= 1 and int(lengths.max()) <= S
    drawn, wanted, gap = oracle_replay(oracle, ann_img, tokens, lengths, gumbel, K, S, SEARCH_T)
    print("ancestral: %d compared draws, smallest top-two key gap %.3e, lengths %s" % (len(drawn), gap, lengths.tolist()))
    assert gap >= 1e-3, "the case's precondition: no near-tie among the oracle's keys (gap %.3e)" % gap
    assert drawn == wanted                                                       # every draw, step 0 and END included; no step is exempt
    assert int((lengths == S).sum()) >= 1 and int((lengths < S).sum()) >= 1      # a cut caption and one that drew END are both here
    ids = ids_for(60)
    for n in range(B * K):
        row = tokens[n].tolist()
        assert all(w not in ids[:3] for w in row[:int(lengths[n])]) and row[0] != ids[3]       # <UNK> is masked at the first step only
        assert all(w == 0 for w in row[int(lengths[n]):])


def test_ancestral_generator_is_reproducible_and_caption_agrees():
    model, _ = tiny()
    img, _, _ = batch(41)
    img = img.cuda()
    kw = dict(beamk=1, max_gen_length=6, temperature=SEARCH_T, sample_method="ancestral")
    a = model.caption_tokens(img, seed=123, **kw)
    b = model.caption_tokens(img, seed=123, **kw)
    c = model.caption_tokens(img, seed=124, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])                                           # 4 x 6 draws over 56 words: another seed, other words
    torch.manual_seed(99)
    seed = int(torch.randint(0, 2 ** 62, (1,)))                                  # the seed caption() will draw from the CPU generator
    want = model.caption_tokens(img, seed=seed, **kw)
    torch.manual_seed(99)
    caps, scores, alphas, ppl = model.caption(img, **kw)
    assert caps == [t[:n] for t, n in zip(want[0].tolist(), want[1].tolist())]


# ---------------------------------------------------------------------------------------------------------------- the whole step
def test_scst_loss_and_every_gradient_against_the_oracle():
    """The net is the residual-damped variant of the tiny model, as in the encoder's own gradient tests.  On the undamped weights the
    fp32 oracle itself is 8.9e-3 (relative L2, encoder.2.weight; every encoder tensor 7e-3 .. 9e-3) from its own fp64 run on this
    loss, one ReLU decision flipping in a batch of 4 pictures with 2 x 2 final maps, and the library measured 7.6e-3 against the fp32
    oracle there with the loss equal to 8 digits: no fp32 evaluation meets 1e-3 on that net.  Damped (0.25), the fp32 oracle is within
    7e-6 of its fp64 run on every tensor, so 1e-3 measures the library (measured: 1.2e-5 at worst, attention.decoder_att.weight)."""
    import sat_amd  # noqa: F401
    from sat_amd import scst
    from oracle import prng, sat_oracle as O
    model, oracle = tiny(damp_residual=0.25)
    B, K, S, T_ = 4, 3, 7, 0.9
    img, _, _ = batch(51)
    ids = ids_for(60)
    model.eval()
    with torch.no_grad():
        ann, _ = model.encode(img.cuda())
        tokens, lens = scst.sample(model, ann.contiguous(), K, S, T_, seed=5)
    # explicit rewards; the greedy baseline with lower scores, so that the advantages of an image's samples do not cancel: with
    # advantages that sum to zero per image the encoder's gradient is a small difference of large terms and its relative norm
    # measures the conditioning of that difference, not the kernels
    scores = torch.from_numpy(prng.uniform((B * K, 2), 61, 0.0, 3.0).astype(np.float64))
    scores_greedy = torch.from_numpy(prng.uniform((B, 2), 62, 0.0, 1.0).astype(np.float64))
    prep = scst.prepare(tokens, lens, scores.cuda(), K, ids, "greedy", (1.0, 0.5), scores_greedy.cuda())
    assert int((prep["advantage"] != 0).sum()) >= 1 and len(set(prep["reward"].tolist())) == B * K
    lengths_host = prep["lengths"].cpu()
    model.train()
    ann_g, _ = model.encode(img.cuda())
    loss = scst.loss(model, ann_g, prep["caps"], lengths_host, prep["step_weight"], None, T_)
    loss.backward()
    # the oracle on the same captions and weights
    caps = prep["caps"].cpu().long().reshape(B, K, S + 2)
    lens_o = lengths_host.long().reshape(B, K)
    sw = prep["step_weight"].cpu()
    count = int(prep["count"].sum())
    ann_o = oracle.encoder(img.clone())
    out = O.decode_train(oracle.sd, oracle.hp, ann_o, caps, lens_o, epsilon=1.0)
    lp, _ = O.pack_time_major(out["logits"], out["lengths"])
    tp, _ = O.pack_time_major(out["targets"], out["lengths"])
    wp, _ = O.pack_time_major(sw, out["lengths"])
    pl, _, _ = R.policy_loss(lp.double(), tp, wp.double(), 1.0 / T_, ids, B * K, 1.0 / max(1, count))
    loss_o = pl.float() + O.doubly_stochastic(out["alphas"], oracle.hp.att_gamma)
    loss_o.backward()
    print("scst loss hip=%.7f oracle=%.7f" % (loss.item(), loss_o.item()))
    assert abs(loss.item() - loss_o.item()) <= 1e-4 * max(1.0, abs(loss_o.item()))
    og = oracle.named_grads()
    worst = {}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        worst[k] = float((p.grad.cpu().double() - og[k].double()).norm()) / max(1e-9, float(og[k].double().norm()))
    for k, e in sorted(worst.items(), key=lambda kv: -kv[1])[:8]:
        print("relative L2 gradient error %-40s %.3e" % (k, e))
    for k, e in worst.items():
        assert e <= 1e-3, "%s: relative L2 gradient error %.3e" % (k, e)


def host_rewards(model_batch, tokens, lengths, K, df, n_images, w):
    """(reward (N) float64, cider, rouge) of the sampled captions on the host (sat_amd/metrics.py)"""
    from sat_amd import metrics
    _, caps, lens = model_batch
    refs = [[c[1:l] for c, l in zip(r, lens[i].tolist())] for i, r in enumerate(caps.tolist())]
    refs_n = [refs[n // K] for n in range(tokens.shape[0])]
    hyps = [t[:n] for t, n in zip(tokens.tolist(), lengths.tolist())]
    cider = metrics.cider_d(refs_n, hyps, df=df, n_images=n_images)
    rouge = [metrics.rouge_l(r, h) for r, h in zip(refs_n, hyps)]
    return np.array([w[0] * c + w[1] * r for c, r in zip(cider, rouge)]), cider, rouge, refs


@pytest.mark.parametrize("baseline", ["mean", "greedy"])
def test_scst_step_end_to_end(baseline):
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E, metrics, scst
    model, _ = tiny()
    model.train()
    b = batch(41)
    gb = (b[0].cuda(), b[1].cuda(), b[2])
    rc = E.ReferenceCorpus(60)
    rc.add(b[1], b[2]); rc.check()
    K, S, w = 3, 7, (1.0, 0.5)
    step0 = model.sat_global_step()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    out = model.scst_step(gb, rc, samples=K, baseline=baseline, reward=w, max_gen_length=S, temperature=0.9, seed=11)
    assert model.training and model.sat_global_step() == step0 + 1               # as training_step counts
    assert set(out) >= {"loss", "reward", "baseline_reward", "advantage_abs", "sample_length"}
    out["loss"].backward()
    assert torch.isfinite(out["loss"]) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    tokens, lengths = out["samples"].cpu(), out["sample_lengths"].cpu()
    df = metrics.document_frequency([[c[1:l] for c, l in zip(r, b[2][i].tolist())] for i, r in enumerate(b[1].tolist())])
    want, cider, rouge, refs = host_rewards(b, tokens, lengths, K, df, 4, w)
    got = out["rewards"].cpu().double().numpy()
    bound = w[0] * CIDER_TOL + w[1] * ROUGE_TOL + 2.0 ** -24 * np.abs(want)
    print("rewards: max|d|=%.3e" % float(np.abs(got - want).max()))
    assert np.all(np.abs(got - want) <= bound), (got, want)
    sg = None
    if baseline == "greedy":
        model.load_state_dict(state)                                             # the batch statistics the step's train-mode pass left behind
        model.eval()
        with torch.no_grad():
            ann, _ = model.encode(gb[0])
            g_tok, g_len = scst.greedy(model, ann, S)
        sg = np.array([[c, r] for c, r in zip(metrics.cider_d(refs, [t[:n] for t, n in zip(g_tok.tolist(), g_len.tolist())], df=df, n_images=4),
                                               [metrics.rouge_l(r, t[:n]) for r, t, n in zip(refs, g_tok.tolist(), g_len.tolist())])])
        model.train()
    ref = R.prepare(tokens.numpy(), lengths.numpy(), np.array([cider, rouge]).T, sg, K, w[0], w[1], R.GREEDY if baseline == "greedy" else R.MEAN,
                    ids_for(60))
    adv = out["advantages"].cpu().double().numpy()
    assert np.all(np.abs(adv - ref["advantage"]) <= 1e-6 * np.maximum(1.0, np.abs(ref["advantage"]))), (adv, ref["advantage"])
    assert abs(float(out["reward"]) - float(want.mean())) <= 1e-6 and abs(float(out["advantage_abs"]) - float(np.abs(ref["advantage"]).mean())) <= 1e-6
    assert abs(float(out["baseline_reward"]) - float(ref["baseline"].mean())) <= 1e-6
    assert abs(float(out["sample_length"]) - float(lengths.float().mean())) <= 1e-6
    model.eval()                                                                 # the flag is restored in eval mode as well
    model.scst_step(gb, rc, samples=K, baseline=baseline, reward=w, max_gen_length=S, seed=12)
    assert not model.training and model.sat_global_step() == step0 + 2


def test_scst_step_bf16_is_finite_and_reproducible():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    model, _ = tiny()
    model.train()
    model.set_precision("bf16")
    b = batch(41)
    gb = (b[0].cuda(), b[1].cuda(), b[2])
    rc = E.ReferenceCorpus(60).add(b[1], b[2])
    state = {k: v.clone() for k, v in model.state_dict().items()}
    runs = []
    for _ in range(2):
        model.load_state_dict(state)                                             # the step's train-mode pass moves the running statistics
        model.zero_grad(set_to_none=True)
        out = model.scst_step(gb, rc, samples=3, baseline="mean", max_gen_length=7, seed=21)
        out["loss"].backward()
        runs.append((out["loss"].detach().clone(), out["samples"].clone(), out["advantages"].clone(), model.output.output.weight.grad.clone()))
    assert torch.isfinite(runs[0][0]) and torch.isfinite(runs[0][3]).all() and torch.isfinite(runs[0][2]).all()
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))


def test_existing_calls_are_bit_equal_around_a_scst_step():
    import sat_amd  # noqa: F401
    from sat_amd import evaluation as E
    model, _ = tiny()
    model.eval()                                                                 # no running statistic moves: what differs would be the step's doing
    for p in model.encoder.parameters():                                         # eval mode and a frozen encoder: the step shares one set of annotations
        p.requires_grad = False
    b = batch(41)
    gb = (b[0].cuda(), b[1].cuda(), b[2])
    rc = E.ReferenceCorpus(60).add(b[1], b[2])

    def existing():
        loss = model.training_step(gb, 0)["loss"].detach().clone()
        torch.manual_seed(7)
        caps = model.caption(gb[0], beamk=3, max_gen_length=7, sample_method="multinomial")
        toks = model.caption_tokens(gb[0], beamk=3, max_gen_length=7, sample_method="multinomial", seed=17)
        return loss, caps[0], caps[1], [t.clone() for t in toks]

    before = existing()
    model.scst_step(gb, rc, samples=3, baseline="greedy", max_gen_length=7, seed=3)["loss"].backward()
    model.zero_grad(set_to_none=True)
    after = existing()
    assert torch.equal(before[0], after[0]) and before[1] == after[1] and before[2] == after[2]
    assert all(torch.equal(x, y) for x, y in zip(before[3], after[3]))
