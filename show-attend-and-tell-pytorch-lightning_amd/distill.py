"""Knowledge distillation (Hinton et al. 2015; DESIGN.md 5, "Distillation"): one student ``SAT`` learns from a teacher ``SAT`` or a whole
``Ensemble``, so that what several models decode together at several models' cost is decoded by one.  The layers, each usable on its own:

``check_step_args``    every ``ValueError`` of ``step`` / ``SAT.distill_step``; touches no GPU
``teacher_logits``     the members' teacher-forced packed logits (P, V) on the batch, under ``torch.no_grad()`` in eval mode
``teacher_captions``   ``targets="teacher"``: the teacher's best beam caption per image as a train batch (sequence-level distillation;
                       Kim & Rush 2016)
``loss``               the student's teacher-forced pass, ``sat_distill_fwd / _bwd`` on the packed logits (include/sat_hip.h) plus the
                       doubly-stochastic term
``step``               the three joined: what ``SAT.distill_step`` runs between its two host halves

The loss is ``(1 - alpha) * CE_smoothed(z, y) + alpha * tau^2 * KL(q || softmax(z / tau))``: ``z`` the student's logits, ``y`` the next word
of the caption both sides are fed, ``q`` the teachers' distributions at temperature ``tau`` combined as the ensemble search combines
them (``Ensemble.weights`` / ``Ensemble.combine``).  Both sides are teacher-forced on the same caption: a student fed its own predictions
would be compared with teachers conditioned on a different prefix."""
import math

import numpy as np
import torch

from . import _lib as L
from . import decoder as Dk
from .ensemble import Ensemble
from .model import SATDecoder
from .scst import special_ids

TARGETS = ("references", "teacher")


def members(teacher):
    """``(models, weights, combine)`` of a teacher: a single model is an ensemble of one"""
    if isinstance(teacher, Ensemble):
        return list(teacher.models), list(teacher.weights), teacher.combine
    if isinstance(teacher, SATDecoder):
        return [teacher], [1.0], "arithmetic"
    raise ValueError("distill: the teacher is a SAT model or an Ensemble, not %r" % (type(teacher).__name__,))


def check_step_args(student, teacher, alpha, temperature, targets, beamk=3, max_gen_length=20):
    """every ``ValueError`` of ``step`` / ``SAT.distill_step``; touches no GPU"""
    models, weights, combine = members(teacher)
    if isinstance(alpha, (list, tuple)) or not (0.0 <= float(alpha) <= 1.0):
        raise ValueError("distill: alpha=%r outside [0, 1]" % (alpha,))
    if isinstance(temperature, (list, tuple)) or not (0.0 < float(temperature) < math.inf):
        raise ValueError("distill: temperature=%r is not one positive finite number" % (temperature,))
    if targets not in TARGETS:
        raise ValueError("distill: targets=%r (%s)" % (targets, " / ".join(TARGETS)))
    if int(beamk) < 1:
        raise ValueError("distill: beamk=%d < 1" % int(beamk))
    if int(max_gen_length) < 1 or int(max_gen_length) + 1 > L.CAPTION_MAX_LEN:
        raise ValueError("distill: max_gen_length=%d outside 1..%d" % (int(max_gen_length), L.CAPTION_MAX_LEN - 1))
    if not 1 <= len(models) <= L.ENSEMBLE_MAX:
        raise ValueError("distill: %d teachers, not 1..%d" % (len(models), L.ENSEMBLE_MAX))
    V, ids = int(student.embedding.weight.shape[0]), special_ids(student)
    for i, m in enumerate(models):
        if m is student:
            raise ValueError("distill: the student is teacher %d (a model does not distil itself)" % i)
        if int(m.embedding.weight.shape[0]) != V:
            raise ValueError("distill: teacher %d has a vocabulary of %d words, the student one of %d" % (i, int(m.embedding.weight.shape[0]), V))
        if special_ids(m) != ids:
            raise ValueError("distill: teacher %d has (START, PAD, END, UNK) = %r, the student %r" % (i, special_ids(m), ids))


class _eval_mode:
    """every member in eval mode inside the block; every module's training flag as it was afterwards"""

    def __init__(self, models):
        self.models = models

    def __enter__(self):
        self.flags = [(mod, mod.training) for m in self.models for mod in m.modules()]
        for m in self.models:
            m.eval()

    def __exit__(self, *exc):
        for mod, flag in self.flags:
            mod.training = flag
        return False


@torch.no_grad()
def teacher_logits(teacher, img, caps, lengths):
    """The members' packed logits ``[(P, V)] * M`` on ``caps (B, R, T)`` / ``lengths (B, R)`` (host): every member encodes ``img`` with its
    own encoder and is teacher-forced through ``train_decode`` in eval mode (no dropout, running statistics untouched).  The rows are in
    the ``PackPlan`` order of ``lengths``, which is the student's.  No member parameter receives a gradient or changes."""
    models = members(teacher)[0]
    T = caps.shape[-1]
    out = []
    with _eval_mode(models):
        for m in models:
            ann, _ = m.encode(img.to(m.embedding.weight.device))
            res = m.train_decode(ann.contiguous(), caps, lengths, with_loss=False, teacher=np.ones(T - 1, np.int32))
            out.append(res["logits_packed"].detach())
    return out


@torch.no_grad()
def teacher_captions(teacher, img, beamk=3, max_gen_length=20):
    """The teacher's best beam caption of every image as a train batch: ``(caps (B, 1, max_gen_length + 2) int64 on the device =
    START, w_1 .. w_len, END, PAD ..., lengths (B, 1) int64 on the HOST = len + 1, the decode steps)``.  One host read: the lengths."""
    models = members(teacher)[0]
    S = int(max_gen_length)
    start, pad, end, _ = special_ids(models[0])
    with _eval_mode(models):
        tokens, lens = teacher.caption_tokens(img, beamk=int(beamk), max_gen_length=S)[:2]
    B = tokens.shape[0]
    tokens = tokens.to(torch.int64)
    ln = lens.to(torch.int64).clamp(1, S).unsqueeze(1)
    j = torch.arange(S + 2, device=tokens.device).unsqueeze(0)
    body = torch.cat([tokens.new_full((B, 1), start), tokens], 1)                        # body[:, j] = tokens[:, j - 1]
    caps = torch.where(j <= ln, body, torch.where(j == ln + 1, torch.full_like(body, end), torch.full_like(body, pad)))
    return caps.reshape(B, 1, S + 2), (ln + 1).cpu()


def loss(student, ann_bld, caps, lengths, teacher_logits, weights, combine, alpha, temperature, return_parts=False):
    """The student's pass.  ``ann_bld (B, L, D)`` (with its graph, when the encoder trains), ``caps (B, R, T)``, ``lengths (B, R)`` on the
    host, ``teacher_logits`` the list ``teacher_logits()`` returned for the same captions (``None`` with ``alpha == 0``, where no teacher
    is read).  The student is teacher-forced through its ordinary ``train_decode`` in the mode the caller left it in; the result is the
    ``DistillFn`` loss (label smoothing: the student's ``label_smoothing``) plus the doubly-stochastic term.  ``return_parts``:
    ``(loss, hard, soft, accuracy)``."""
    T = caps.shape[-1]
    res = student.train_decode(ann_bld, caps, lengths, with_loss=False, teacher=np.ones(T - 1, np.int32))
    logits = res["logits_packed"]
    if teacher_logits is None:
        if float(alpha) != 0.0:
            raise ValueError("distill.loss: alpha=%r needs teacher_logits" % (alpha,))
        teacher_logits, weights = [logits.detach()], [1.0]                               # a (P, V) pointer the kernel does not read
    targets = res["targets_packed"].to(torch.int32).contiguous()
    dl, hard, soft, acc = Dk.DistillFn.apply(logits, targets, list(teacher_logits), list(weights), combine, 1.0 / float(temperature), float(alpha),
                                             float(student.criterion.smoothing))
    total = dl + student.attention_term(res["alphas"])
    return (total, hard, soft, acc) if return_parts else total


def step(student, batch, teacher, alpha=0.5, temperature=2.0, targets="references", beamk=3, max_gen_length=20):
    """One distillation step without the optimizer bookkeeping (``SAT.distill_step`` adds it).  ``batch``: ``training_step``'s (img,
    captions (B, R, T), lengths (B, R)).  The teacher's passes run under ``torch.no_grad()`` in eval mode and every training flag is
    restored; the student's pass is its ordinary path in the mode the caller left it in.  ``targets="teacher"`` replaces the references
    by the teacher's best beam caption (``beamk``, ``max_gen_length``), one caption per image, at the cost of one host read of its
    lengths.  Returns ``{"loss", "hard", "soft", "accuracy"}``: the loss to back-propagate, the mean label-smoothed cross entropy, the
    mean unscaled KL and the student's next-word accuracy, device scalars."""
    check_step_args(student, teacher, alpha, temperature, targets, beamk, max_gen_length)
    img, caps, lengths = batch
    dev = student.embedding.weight.device
    img = img.to(dev)
    _, weights, combine = members(teacher)
    if targets == "teacher":
        caps, lengths = teacher_captions(teacher, img, beamk, max_gen_length)
    tl = teacher_logits(teacher, img, caps, lengths) if float(alpha) != 0.0 else None
    ann, _ = student.encode(img)
    total, hard, soft, acc = loss(student, ann, caps, lengths, tl, weights, combine, alpha, temperature, return_parts=True)
    return {"loss": total, "hard": hard, "soft": soft, "accuracy": acc}
