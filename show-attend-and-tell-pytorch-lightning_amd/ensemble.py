"""Ensemble decoding ("Ensemble decoding"): one batched beam search over several captioning models.

``Ensemble(models, weights, combine)`` stands where ``evaluation.py`` and the tools expect a model: every member (a whole ``SAT`` /
``SATDecoder`` with its own encoder, sizes, layer count, ``deep_output`` and precision; one shared vocabulary) is fed the same token
history, the members' per-step distributions are combined on the device (``sat_beam_search_ensemble``, include/sat_hip.h) and ONE
selection keeps the hypotheses.  ``combine="arithmetic"`` mixes the distributions, ``"geometric"`` multiplies them (a product of
experts, renormalised).  "beam" sampling with temperature lists, banned ids / ``no_unk``, ``min_length`` and ``no_repeat_ngram``; every
``rescore_method``.  The weights are given, not learned."""
import ctypes as C
import inspect
import math

import torch

from . import _lib as L
from . import constraints
from . import decoder as Dk
from .model import SAT, SATDecoder

COMBINE = tuple(L.ENSEMBLE_COMBINE)


class Annotations(list):
    """``Ensemble.encode``'s first result: the members' annotations (B, L_i, D_i), a list that answers what the search surface asks of
    one annotation tensor"""

    @property
    def shape(self):
        return self[0].shape

    def contiguous(self):
        return Annotations(a.contiguous() for a in self)


def _bound(fn, args, kw):
    """the arguments of ``fn(self, *args, **kw)`` by name, defaults filled in (``fn``: the ``SAT`` method of the same name)"""
    b = inspect.signature(fn).bind(None, *args, **kw)
    b.apply_defaults()
    a = dict(b.arguments)
    a.pop("self", None)
    return a


def check_decode_args(sample_method="beam", topg=None, prefix=None, repetition_penalty=None, beam_groups=None, decoder_noise=None, graph=False, required=None, **_):
    """``ValueError`` for every keyword an ensemble does not decode with, each naming its argument.  Touches no GPU."""
    if str(sample_method) != "beam":
        raise ValueError("an ensemble decodes with sample_method='beam' only, not %r" % (sample_method,))
    if topg is not None:
        raise ValueError("an ensemble does not combine with topg=%r" % (topg,))
    if prefix is not None:
        raise ValueError("an ensemble does not combine with a forced prefix (prefix=%r)" % (prefix,))
    if repetition_penalty is not None and float(repetition_penalty) != 1.0:
        raise ValueError("an ensemble does not combine with repetition_penalty=%r (the members' raw logits are not one model's)" % (repetition_penalty,))
    if beam_groups is not None and int(beam_groups) not in (0, 1):
        raise ValueError("an ensemble does not combine with beam_groups=%r" % (beam_groups,))
    if decoder_noise:
        raise ValueError("an ensemble does not combine with decoder_noise=%r" % (decoder_noise,))
    if graph:
        raise ValueError("an ensemble search is not replayed from a graph (graph=True)")
    if required is not None and len(required) > 0 and (isinstance(required, str) or torch.is_tensor(required) or any(
            not isinstance(r, (str, list, tuple)) or len(r) > 0 for r in required)):
        raise ValueError("an ensemble does not search with required words (required=%r)" % (required,))


class Ensemble:
    def __init__(self, models, weights=None, combine="arithmetic"):
        models = list(models)
        if not 1 <= len(models) <= L.ENSEMBLE_MAX:
            raise ValueError("an ensemble has 1..%d members, not %d" % (L.ENSEMBLE_MAX, len(models)))
        if combine not in L.ENSEMBLE_COMBINE:
            raise ValueError("combine=%r is none of %r" % (combine, COMBINE))
        for i, m in enumerate(models[1:], 1):
            if dict(m.hp.vocab_stoi) != dict(models[0].hp.vocab_stoi) or m.embedding.weight.shape[0] != models[0].embedding.weight.shape[0]:
                raise ValueError("member %d does not share member 0's vocabulary (vocab_stoi and vocabulary size must be equal)" % i)
        if weights is None:
            weights = [1.0] * len(models)
        try:
            weights = [float(w) for w in weights]
        except (TypeError, ValueError):
            raise ValueError("weights=%r is not a list of numbers" % (weights,))
        if len(weights) != len(models):
            raise ValueError("%d weights for %d members" % (len(weights), len(models)))
        if not all(math.isfinite(w) and w >= 0.0 for w in weights):
            raise ValueError("weights=%r: every weight is a finite number >= 0" % (weights,))
        total = math.fsum(weights)
        if not total > 0.0:
            raise ValueError("weights=%r: every weight is 0" % (weights,))
        self.models, self.weights, self.combine = models, [w / total for w in weights], combine

    @classmethod
    def from_checkpoints(cls, paths, weights=None, combine="arithmetic", device="cuda"):
        """the ensemble of the ``SAT`` models saved at ``paths`` (``hyper_parameters`` + ``state_dict``, as tools/evaluate.py reads them)"""
        models = []
        for path in paths:
            ckpt = torch.load(path, map_location="cpu", weights_only=False)
            model = SAT(**dict(ckpt["hyper_parameters"]))
            model.load_state_dict(ckpt["state_dict"])
            models.append(model.to(device))
        return cls(models, weights, combine)

    # ------------------------------------------------------------------ what evaluation.py asks of a model
    @property
    def hp(self):
        return self.models[0].hp

    hparams = hp

    @property
    def pad_idx(self):
        return self.models[0].pad_idx

    @property
    def embedding(self):
        return self.models[0].embedding

    def eval(self):
        for m in self.models:
            m.eval()
        return self

    def decode_seq(self, seq, remove_special=False):
        return self.models[0].decode_seq(seq, remove_special)

    def encode(self, img):
        """(the members' annotations, member 0's (h, w)): the maps a search returns are member 0's"""
        enc = [m.encode(img) for m in self.models]
        return Annotations(a for a, _ in enc), enc[0][1]

    def _single(self):
        return self.models[0] if len(self.models) == 1 else None

    def _check(self, a, batch_size=None):
        """every refusal of a decode call, before any launch"""
        check_decode_args(**a)
        if int(a["max_gen_length"]) < 1:
            raise ValueError("an ensemble runs in the batched search only (max_gen_length >= 1), not in the per-image loop beam_decode")
        V = self.embedding.weight.shape[0]
        if batch_size is not None:
            constraints.SearchOptions.from_kwargs(a).resolve(self.hp.vocab_stoi, V, batch_size, a["beamk"], a["max_gen_length"])
        if "mbr_corpus" in a:
            corpus = a["mbr_corpus"] if a["mbr_corpus"] is not None else a.get("corpus")
            constraints.check_mbr(a.get("rescore_method"), corpus, a["mbr_reward"], a["mbr_alpha"], a["beamk"], V, a["max_gen_length"])

    def _beam_search_device(self, ann_bld, beamk, max_gen_length, temperature, sample_method="beam", sample_topk=3, decoder_noise=None, seed=None, gumbel=None,
                            normals=None, graph=False, topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None,
                            min_length=None, repetition_penalty=None, beam_groups=None, diversity_penalty=0.5, required=None, options=None):
        """``SATDecoder._beam_search_device`` for the ensemble: ``ann_bld`` is the list of the members' annotations (B, L_i, D_i); the
        same dict of device buffers comes back (``alpha_hist`` holds member 0's maps).  Launches only."""
        opt = options if options is not None else constraints.SearchOptions.from_kwargs(locals())
        check_decode_args(**opt.kwargs(check_decode_args))
        one = self._single()
        if one is not None:
            ann = ann_bld[0] if isinstance(ann_bld, (list, tuple)) else ann_bld
            return one._beam_search_device(ann, beamk, max_gen_length, temperature, options=opt)
        anns = [a.contiguous() for a in ann_bld]
        if len(anns) != len(self.models):
            raise ValueError("%d annotation tensors for %d members" % (len(anns), len(self.models)))
        B = anns[0].shape[0]
        if any(a.dim() != 3 or a.shape[0] != B for a in anns):
            raise ValueError("every member's annotations are (B, L_i, D_i) of the same B images")
        V = self.embedding.weight.shape[0]
        K, S = int(beamk), int(max_gen_length)
        con, hist, _, _ = opt.resolve(self.hp.vocab_stoi, V, B, K, S)
        L.require_gpu(*anns)
        dev = anns[0].device
        ens = L.BeamEnsemble(members=len(self.models), combine=L.ENSEMBLE_COMBINE[self.combine])
        keep = [ens]
        for i, (m, ann, wt) in enumerate(zip(self.models, anns, self.weights)):
            _, Lc, D = ann.shape
            dims = Dk.decoder_dims(B, K, 2, Lc, D, m.attention.decoder_att.weight.shape[0], m.embedding.weight.shape[1], m.lstm.weight_hh_l0.shape[1], V, 0,
                                   m.hp.deep_output, m.pad_idx, int(getattr(m, "sat_precision", "fp32") == "bf16"), layers=int(m.hp.decoder_layers))
            w, tens = m._params_struct()
            keep += [dims, w, tens]
            ens.dims[i], ens.params[i], ens.ann[i], ens.weight[i] = C.pointer(dims), C.pointer(w), ann.data_ptr(), wt
        desc = Dk.search_desc(self.hp.vocab_stoi, K, S, temperature, dev, con, hist)
        desc.ensemble = C.pointer(ens)
        desc._keep += keep
        return Dk.beam_search(desc, B, anns[0].shape[1], dev)

    def beam_decode_batched(self, ann_bld, hw, *args, **kw):
        """``SATDecoder.beam_decode_batched`` (same arguments, same four lists) on the list of the members' annotations"""
        a = _bound(SATDecoder.beam_decode_batched, (ann_bld, hw) + args, kw)
        self._check(a, a["ann_bld"][0].shape[0] if isinstance(ann_bld, (list, tuple)) else ann_bld.shape[0])
        one = self._single()
        if one is not None:
            return one.beam_decode_batched(ann_bld[0] if isinstance(ann_bld, (list, tuple)) else ann_bld, hw, *args, **kw)
        return SATDecoder.beam_decode_batched(self, Annotations(ann_bld), hw, *args, **kw)

    @torch.no_grad()
    def caption(self, img_tensor, *args, **kw):
        """``SAT.caption`` (same arguments): (captions, scores, member 0's attention maps, perplexities); ``return_all`` and every
        ``rescore_method``, "MBR" included"""
        a = _bound(SAT.caption, (img_tensor,) + args, kw)
        self._check(a, img_tensor.shape[0])
        one = self._single()
        if one is not None:
            return one.caption(img_tensor, *args, **kw)
        self.eval()
        ann, hw = self.encode(img_tensor)
        names = set(inspect.signature(SATDecoder.beam_decode_batched).parameters)
        return SATDecoder.beam_decode_batched(self, ann.contiguous(), hw, **{k: v for k, v in a.items() if k in names})

    forward = caption
    __call__ = caption

    def score_captions(self, captions, encoded_captions, lengths, perplexities=None):
        """``SAT.score_captions`` through member 0 (its embedding table measures the cosine similarity)"""
        return self.models[0].score_captions(captions, encoded_captions, lengths, perplexities)

    def val_batch(self, batch, *args, **kw):
        a = _bound(SAT.val_batch, (batch,) + args, kw)
        self._check(a, batch[0].shape[0])
        return SAT.val_batch(self, batch, *args, **kw)

    def caption_tokens(self, img, *args, **kw):
        from . import evaluation
        a = _bound(SAT.caption_tokens, (img,) + args, kw)
        self._check(a, img.shape[0])
        one = self._single()
        if one is not None:
            return one.caption_tokens(img, *args, **kw)
        return evaluation.caption_tokens(self, img, **{k: v for k, v in a.items() if k != "img"})

    def val_batch_stats(self, batch, *args, **kw):
        from . import evaluation
        a = _bound(SAT.val_batch_stats, (batch,) + args, kw)
        self._check(a, batch[0].shape[0])
        one = self._single()
        if one is not None:
            return one.val_batch_stats(batch, *args, **kw)
        return evaluation.val_batch_stats(self, batch, **{k: v for k, v in a.items() if k != "batch"})

    def visualize(self, items, *args, **kw):
        """``SAT.visualize`` (same arguments): the overlays are member 0's attention along the ensemble's captions"""
        from . import visualize
        a = _bound(SAT.visualize, (items,) + args, kw)
        render = a.pop("render", {})
        self._check(dict(a, **render), len(items))
        one = self._single()
        if one is not None:
            return one.visualize(items, *args, **kw)
        return visualize.visualize(self, items, **{k: v for k, v in a.items() if k != "items"}, **render)

    def caption_image(self, items, *args, **kw):
        from . import visualize
        a = _bound(SAT.caption_image, (items,) + args, kw)
        self._check(a, len(items))
        one = self._single()
        if one is not None:
            return one.caption_image(items, *args, **kw)
        return visualize.caption_image(self, items, **{k: v for k, v in a.items() if k != "items"})
