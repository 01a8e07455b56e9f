"""Self-critical sequence training (SCST; Rennie et al. 2017) on the on-device CIDEr-D / ROUGE-L reward ("Self-critical
training").  The layers, each usable on its own:

``sample``   K ancestral samples per image from the batched search (``sample_method="ancestral"``, every word drawn from the model's
             own distribution over the unmasked words), left on the device
``greedy``   the beam-1 caption of every image (the greedy baseline)
``rewards``  ``evaluation.consensus_scores`` with the references repeated per sample
``prepare``  ``sat_scst_prepare``: rewards, advantages and the train batch (captions, lengths, per-step weights) in one launch
``loss``     the teacher-forced gradient pass over the sampled captions: ``sat_policy_nll_fwd / _bwd`` on the packed logits plus the
             doubly-stochastic term
``step``     the five joined: what ``SAT.scst_step`` runs between its two host halves

The estimator is REINFORCE with a baseline: ``grad = -E[(r(w) - b) * grad log q(w)]`` with ``q`` the distribution the sampler draws from,
i.e. the softmax at the search's temperature renormalised over the words the search leaves unmasked ({START, PAD} always, {END, UNK} as
well at the first step).  A sample the search cut at ``max_gen_length`` words has no END action: that step's weight is zero."""
import math

import numpy as np
import torch

from . import _lib as L
from . import decoder as Dk
from . import evaluation

BASELINES = tuple(L.SCST_BASELINES)
SPECIALS = ("<START>", "<PAD>", "<END>", "<UNK>")


def special_ids(model):
    """(START, PAD, END, UNK) as host ints"""
    return tuple(int(model.hp.vocab_stoi[s]) for s in SPECIALS)


def _masked_ids(model, dev):
    """the four ids as a device int32 tensor, uploaded once per (model, device)"""
    cache = model.__dict__.setdefault("_scst_masked_ids", {})
    t = cache.get(str(dev))
    if t is None:
        t = cache[str(dev)] = torch.tensor(special_ids(model), dtype=torch.int32, device=dev)
    return t


def check_step_args(model, corpus, samples, baseline, reward, max_gen_length, temperature):
    """every ``ValueError`` of ``step`` / ``SAT.scst_step``; touches no GPU"""
    if corpus is None or getattr(corpus, "images", 0) < 1:
        raise ValueError("scst: a ReferenceCorpus that holds the split's references is required (corpus=%r)" % (corpus,))
    if baseline not in BASELINES:
        raise ValueError("scst: baseline=%r (%s)" % (baseline, " / ".join(BASELINES)))
    K, S = int(samples), int(max_gen_length)
    if K < 1 or K > L.SCST_MAX_SAMPLES:
        raise ValueError("scst: samples=%d outside 1..%d" % (K, L.SCST_MAX_SAMPLES))
    if baseline == "mean" and K < 2:
        raise ValueError("scst: baseline='mean' is the mean reward of the other samples of the image: samples >= 2 (samples=%d)" % K)
    if int(model.hp.vocab_size) > evaluation.MAX_VOCAB:
        raise ValueError("scst: vocab_size=%d above %d (the n-gram keys of the reward)" % (int(model.hp.vocab_size), evaluation.MAX_VOCAB))
    if S < 1 or S + 1 > L.CAPTION_MAX_LEN:
        raise ValueError("scst: max_gen_length=%d outside 1..%d" % (S, L.CAPTION_MAX_LEN - 1))
    if isinstance(temperature, (list, tuple)) or not (0.0 < float(temperature) < math.inf):
        raise ValueError("scst: temperature=%r is not one positive finite number" % (temperature,))
    if len(reward) != 2 or not all(math.isfinite(float(w)) for w in reward):
        raise ValueError("scst: reward=%r is not (w_cider, w_rouge), two finite weights" % (reward,))


@torch.no_grad()
def sample(model, ann_bld, samples, max_gen_length, temperature=1.0, seed=None, gumbel=None):
    """``samples`` independent ancestral samples of every image of ``ann_bld (B, L, D)``: ``(tokens (B * samples, max_gen_length + 1) int32
    padded with <PAD>, lengths (B * samples) int32)`` on the device, image b owning rows ``b * samples ...``.  The samples are rows of a
    ``B * samples``-image batch searched with one hypothesis each.  ``gumbel``: an optional table (max_gen_length + 1, B * samples, V)
    in place of the device generator seeded by ``seed``."""
    K = int(samples)
    if K < 1:
        raise ValueError("scst.sample: samples=%d" % K)
    ann = ann_bld.repeat_interleave(K, 0).contiguous()
    o = model._beam_search_device(ann, 1, int(max_gen_length), float(temperature), sample_method="ancestral", seed=seed, gumbel=gumbel)
    sel = evaluation.select_hypotheses(o, model.pad_idx)
    return sel["tokens"], sel["lengths"]


@torch.no_grad()
def greedy(model, ann_bld, max_gen_length):
    """the beam-1 caption of every image: ``(tokens (B, max_gen_length + 1), lengths (B))`` on the device"""
    o = model._beam_search_device(ann_bld.contiguous(), 1, int(max_gen_length), 1.0)
    sel = evaluation.select_hypotheses(o, model.pad_idx)
    return sel["tokens"], sel["lengths"]


def rewards(tokens, lengths, refs, ref_lengths, corpus, samples=1):
    """``(N, 2)`` float64 ``[CIDEr-D, ROUGE-L]`` of ``tokens (N, W)`` with ``N = B * samples`` against ``refs (B, R, T)`` /
    ``ref_lengths (B, R)`` (int32, on the device), image b's references serving its ``samples`` rows"""
    K = int(samples)
    if K > 1:
        refs, ref_lengths = refs.repeat_interleave(K, 0).contiguous(), ref_lengths.repeat_interleave(K, 0).contiguous()
    return evaluation.consensus_scores(tokens, lengths, refs, ref_lengths, corpus)


def prepare(tokens, lengths, scores, samples, ids, baseline="mean", reward=(1.0, 0.0), scores_greedy=None):
    """``sat_scst_prepare`` (include/sat_hip.h): from ``tokens (N, S + 1)`` / ``lengths (N)`` / ``scores (N, 2)`` float64 (and
    ``scores_greedy (B, 2)`` for ``baseline="greedy"``) to ``dict(reward (N), baseline (N), advantage (N), caps (N, S + 2) int32,
    lengths (N) int32 = decode steps, step_weight (N, S + 1), count (N) int32)`` on the device.  ``ids``: (START, PAD, END, UNK) host ints."""
    import ctypes as C
    if baseline not in L.SCST_BASELINES:
        raise ValueError("scst.prepare: baseline=%r (%s)" % (baseline, " / ".join(BASELINES)))
    K = int(samples)
    if baseline == "mean" and K < 2:
        raise ValueError("scst.prepare: baseline='mean' needs samples >= 2 (samples=%d)" % K)
    if baseline == "greedy" and scores_greedy is None:
        raise ValueError("scst.prepare: baseline='greedy' needs scores_greedy")
    L.require_gpu(tokens, lengths, scores, scores_greedy)
    N, W = tokens.shape
    if K < 1 or N % K or tuple(scores.shape) != (N, 2) or lengths.numel() != N:
        raise ValueError("scst.prepare: %d rows for %d samples per image, scores %s, %d lengths" % (N, K, tuple(scores.shape), lengths.numel()))
    B, S = N // K, W - 1
    assert tokens.dtype == torch.int32 and lengths.dtype == torch.int32 and scores.dtype == torch.float64
    tokens, lengths, scores = tokens.contiguous(), lengths.contiguous(), scores.contiguous()
    if scores_greedy is not None:
        assert scores_greedy.dtype == torch.float64 and tuple(scores_greedy.shape) == (B, 2)
        scores_greedy = scores_greedy.contiguous()
    dev = tokens.device
    i32 = dict(dtype=torch.int32, device=dev); f32 = dict(dtype=torch.float32, device=dev)
    out = dict(reward=torch.empty(N, **f32), baseline=torch.empty(N, **f32), advantage=torch.empty(N, **f32), caps=torch.empty(N, S + 2, **i32),
               lengths=torch.empty(N, **i32), step_weight=torch.empty(N, S + 1, **f32), count=torch.empty(N, **i32))
    idarr = (C.c_int32 * 4)(*[int(i) for i in ids])
    L.check(L.lib().sat_scst_prepare(L.ptr(tokens), L.ptr(lengths), L.ptr(scores), L.ptr(scores_greedy), B, K, S, float(reward[0]), float(reward[1]),
                                     L.SCST_BASELINES[baseline], idarr, L.ptr(out["reward"]), L.ptr(out["baseline"]), L.ptr(out["advantage"]),
                                     L.ptr(out["caps"]), L.ptr(out["lengths"]), L.ptr(out["step_weight"]), L.ptr(out["count"]), L.stream_ptr()),
            "sat_scst_prepare")
    return out


def loss(model, ann_bld, caps, lengths, step_weight, count=None, temperature=1.0):
    """The gradient pass.  ``ann_bld (B, L, D)`` (with its graph, when the encoder trains), ``caps (N, T)`` / ``step_weight (N, T - 1)`` on
    the device and ``lengths (N)`` on the HOST (the packing plan needs them), ``N = B * samples``, as ``prepare`` returns them.  The
    sampled captions are teacher-forced through the model's ordinary ``train_decode`` (in train mode with dropout on, that pass's
    distribution differs from the sampler's: the usual approximation); the loss is
    ``-(1 / max(1, sum count)) * sum over the packed steps of step_weight * log q(word)`` plus the doubly-stochastic term, ``q`` the
    softmax of ``logits / temperature`` over the unmasked words.  ``count``: host or device (N); by default it is taken from the host
    lengths (``len + (len < S)``), which costs no device read."""
    N, T = caps.shape
    B = ann_bld.shape[0]
    if N % B:
        raise ValueError("scst.loss: %d captions for %d images" % (N, B))
    lens = torch.as_tensor(lengths).reshape(-1).cpu().to(torch.int64)
    if count is None:
        words = lens - 1
        total = int((words + (words < T - 2).to(torch.int64)).sum())
    else:
        total = int(torch.as_tensor(count).sum())
    res = model.train_decode(ann_bld, caps.reshape(B, N // B, T), lens.reshape(B, N // B), with_loss=False, teacher=np.ones(T - 1, np.int32))
    plan = res["plan"]
    weight = plan.pack(step_weight.to(torch.float32).unsqueeze(-1)).squeeze(-1).contiguous()
    targets = res["targets_packed"].to(torch.int32).contiguous()
    n_first = int(plan.batch_sizes[0]) if plan.batch_sizes.numel() else 0            # the rows of decode step 0 come first: all N captions
    pl = Dk.PolicyNLLFn.apply(res["logits_packed"], targets, weight, 1.0 / float(temperature), _masked_ids(model, ann_bld.device), n_first,
                              1.0 / max(1, total))
    return pl + model.attention_term(res["alphas"])


def step(model, batch, corpus, samples=5, baseline="mean", reward=(1.0, 0.0), max_gen_length=20, temperature=1.0, seed=None):
    """One self-critical step without the optimizer bookkeeping (``SAT.scst_step`` adds it).  Sampling, the baseline and the scoring
    run under ``torch.no_grad()`` in eval mode, as ``caption_tokens`` does, and the training flag is restored; the gradient pass is the
    model's ordinary path in the mode the caller left it in.  When the module is in eval mode and no encoder parameter requires a
    gradient, the annotations are computed once and shared by both halves.  One host read: the ``B * samples`` sampled lengths."""
    check_step_args(model, corpus, samples, baseline, reward, max_gen_length, temperature)
    img, refs, ref_lengths = batch
    dev = model.embedding.weight.device
    img = img.to(dev)
    K, S = int(samples), int(max_gen_length)
    was_training = model.training
    try:
        model.eval()
        with torch.no_grad():
            ann, _ = model.encode(img)
            ann = ann.contiguous()
            tokens, lens = sample(model, ann, K, S, temperature, seed)
            refs_d = torch.as_tensor(refs).to(device=dev, dtype=torch.int32).contiguous()
            rl_d = torch.as_tensor(ref_lengths).to(device=dev, dtype=torch.int32).contiguous()
            scores = rewards(tokens, lens, refs_d, rl_d, corpus, K)
            scores_greedy = None
            if baseline == "greedy":
                g_tokens, g_lens = greedy(model, ann, S)
                scores_greedy = rewards(g_tokens, g_lens, refs_d, rl_d, corpus, 1)
            prep = prepare(tokens, lens, scores, K, special_ids(model), baseline, reward, scores_greedy)
    finally:
        model.train(was_training)
    lengths_host = prep["lengths"].cpu()                                                   # the one host read of the step
    if was_training or any(p.requires_grad for p in model.encoder.parameters()):
        ann, _ = model.encode(img)
    out = dict(loss=loss(model, ann, prep["caps"], lengths_host, prep["step_weight"], None, temperature),
               reward=prep["reward"].mean(), baseline_reward=prep["baseline"].mean(), advantage_abs=prep["advantage"].abs().mean(),
               sample_length=lens.float().mean(), samples=tokens, sample_lengths=lens, rewards=prep["reward"], advantages=prep["advantage"])
    return out
