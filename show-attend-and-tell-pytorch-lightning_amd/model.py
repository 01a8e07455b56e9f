"""Drop-in mirror of the reference's ``model.py`` surface for the train-step hot path:
``get_encoder``, ``InitLSTM``, ``SoftAttention``, ``DeepOutput`` and ``SAT`` with the same
constructor kwargs, attribute names and state-dict keys (reference model.py:16-199),
so ``train.py``-style callers and checkpoints keep working.  The sub-modules (modules.py) hold the
parameters (created in the reference's order, so a given seed yields the same initial weights) and
are callable with the reference's signatures; ``train_batch`` runs the whole decode loop fused in
the library instead of calling them step by step.  All arithmetic goes through ``libsat_hip.so``.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch import nn

from torch.nn.utils.rnn import PackedSequence
from torch.optim.lr_scheduler import MultiStepLR, ReduceLROnPlateau, ExponentialLR, CosineAnnealingWarmRestarts, OneCycleLR

from . import _lib as L
from . import constraints
from . import decoder as Dk
from . import encoder as E
from .modules import DeepOutput, Embedding, Gate, InitLSTM, LSTM, LSTMLayerNorm, SoftAttention  # noqa: F401  (the reference's module names, model.py:66-131)
from .encoder import get_encoder  # noqa: F401  (module-level name, as in the reference)

try:                                     # Lightning is optional plumbing (absent in the build image)
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:                        # pragma: no cover - exercised where Lightning is missing
    pl = None
    _Base = nn.Module


class _HParams(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    __setattr__ = dict.__setitem__


class LabelSmoothing(nn.Module):
    """util.py:91-112 on the HIP kernel; ``forward`` returns the loss, ``last_accuracy`` the
    argmax accuracy of the same rows (model.py:596-597) computed in the same pass."""

    def __init__(self, smoothing=0.0):
        super().__init__()
        self.confidence, self.smoothing = 1.0 - smoothing, smoothing
        self.last_accuracy = None

    def forward(self, x, target):
        loss, acc = Dk.LabelSmoothingFn.apply(x, target.to(torch.int32), self.smoothing)
        self.last_accuracy = acc
        return loss


class TokenLoss(nn.Module):
    """The token losses on the HIP kernel ("Token losses"; ``Dk.TokenLossFn``): ``token_loss`` in "ce" / "fl" / "ce+fl"
    chooses label-smoothed cross entropy, focal loss (Lin et al. 2017, ``focal_gamma``) or their sum; ``ul_alpha`` > 0 adds token-level
    unlikelihood (Welleck et al. 2019) against the words the ground-truth caption has already said.  ``forward(x, target, context)``
    returns the loss; ``context`` = (captions (N, T) int32 on the device, the ``PackPlan`` of ``x``'s rows) is needed when ``ul_alpha``
    > 0.  ``last_accuracy`` is ``LabelSmoothing``'s, ``last_terms`` the dict of the unweighted means "ce" / "fl" / "ul" / "repeat_mass"
    (detached device scalars; a term that is off is 0)."""

    TERMS = ("ce", "fl", "ul", "repeat_mass")

    def __init__(self, smoothing=0.0, token_loss="ce", focal_gamma=2.0, ul_alpha=0.0, pad_id=None):
        super().__init__()
        if token_loss not in L.TOKEN_LOSSES:
            raise ValueError("token_loss=%r is none of %r" % (token_loss, tuple(L.TOKEN_LOSSES)))
        for k, v in (("focal_gamma", focal_gamma), ("ul_alpha", ul_alpha)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError("%s=%r: a finite number >= 0" % (k, v))
        self.confidence, self.smoothing = 1.0 - smoothing, smoothing
        self.token_loss, self.focal_gamma, self.ul_alpha = token_loss, float(focal_gamma), float(ul_alpha)
        self.ce_weight, self.focal_weight = L.TOKEN_LOSSES[token_loss]
        self.pad_id = pad_id
        self.last_accuracy = None
        self.last_terms = None

    def fn_args(self, context):
        """the arguments of ``Dk.TokenLossFn`` behind (logits, targets): graph.py calls its forward with the same ones"""
        caps_i32 = src_row = None
        if self.ul_alpha:
            if context is None:
                raise ValueError("TokenLoss: ul_alpha=%g needs context=(captions, plan)" % self.ul_alpha)
            caps_i32, src_row = context[0], context[1].src_row
        return (self.smoothing, self.ce_weight, self.focal_weight, self.focal_gamma, self.ul_alpha, caps_i32, src_row, self.pad_id)

    def keep(self, acc, terms):
        self.last_accuracy = acc
        self.last_terms = {k: terms[i] for i, k in enumerate(self.TERMS)}

    def forward(self, x, target, context=None):
        loss, acc, terms = Dk.TokenLossFn.apply(x, target.to(torch.int32), *self.fn_args(context))
        self.keep(acc, terms)
        return loss


SAMPLE_METHODS = tuple(L.SAMPLE_METHODS)


def _named(kw):
    """a method's own arguments (its ``locals()`` on entry) by name, for the function that takes the same keywords"""
    return {k: v for k, v in kw.items() if k != "self"}


check_sample_topp = constraints.check_sample_topp
check_ancestral = constraints.check_ancestral


def nucleus_candidates(scores, topp, with_margin=False):
    """The candidates of "nucleus" sampling ("Sampled decoding") for scores (k, V), in torch ops: per row the finite
    entries ordered by (-score, id) (a stable sort), their weights exp(s - max) summed cumulatively in float64, cut at the shortest
    leading run that reaches ``topp`` of the total (``topp >= 1`` or a run that never reaches it: every finite entry).  Returns the
    flat indices row * V + word, rows in order and each row's words in sorted order; with ``with_margin`` also, per row, how far
    the cumulative share at the cut and just before it (a run of equal scores around the cut counting as one position) lies from
    ``topp``: the distance by which rounding would have to move a sum to change the set (inf where nothing is cut)."""
    k, V = scores.shape
    sv, si = torch.sort(scores, dim=1, descending=True, stable=True)
    fin = torch.isfinite(sv)
    svd = sv.double()
    w = torch.where(fin, torch.exp(svd - svd[:, :1]), torch.zeros((), dtype=torch.float64, device=scores.device))
    cum = w.cumsum(1)
    total = w.sum(1, keepdim=True)
    n_fin = fin.sum(1)
    reach = (cum >= float(topp) * total) & fin
    count = torch.where(reach.any(1), reach.to(torch.int64).argmax(1) + 1, n_fin)
    if float(topp) >= 1.0:
        count = n_fin
    member = torch.arange(V, device=scores.device).unsqueeze(0) < count.unsqueeze(1)
    cand = (si + (torch.arange(k, device=scores.device) * V).unsqueeze(1))[member]
    if not with_margin:
        return cand
    margins = []
    svc, share, cnt = sv.cpu(), (cum / total).cpu(), count.tolist()
    for r in range(k):
        if float(topp) >= 1.0 or cnt[r] == 0:
            margins.append(float("inf")); continue
        a = b = cnt[r] - 1                                  # the cut position, widened to the run of scores equal to it
        while a > 0 and svc[r, a - 1] == svc[r, a]:
            a -= 1
        while b + 1 < V and svc[r, b + 1] == svc[r, b]:
            b += 1
        m = abs(float(share[r, b]) - float(topp))
        if a > 0:
            m = min(m, abs(float(share[r, a - 1]) - float(topp)))
        margins.append(m)
    return cand, margins


class SATDecoder(nn.Module):
    """Everything of ``SAT`` except the encoder (model.py:146-199): the decoder parameters under
    the reference's names and the fused train-time decode."""

    def __init__(self, hp):
        super().__init__()
        self._build_decoder(hp)

    def _build_decoder(self, hp, encoder_factory=None):
        if isinstance(hp, dict) and not isinstance(hp, _HParams):
            hp = _HParams(hp)
        self.hp = hp
        if not 1 <= hp.decoder_layers <= L.MAX_LSTM_LAYERS:
            raise NotImplementedError("HIP decoder: decoder_layers=%d (the library stacks 1..%d LSTM layers)" % (hp.decoder_layers, L.MAX_LSTM_LAYERS))
        assert 0 <= hp.label_smoothing < (hp.vocab_size - 1) / hp.vocab_size
        for k in ("ar_alpha", "tar_beta"):                  # activation regularisation: coefficients of ar / tar in training_step's loss
            v = getattr(hp, k, 0.0)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError("%s=%r: a finite coefficient >= 0 (0: off)" % (k, v))
        Dk.check_weight_drop(getattr(hp, "weight_drop", 0.0))      # weight-drop and variational dropout: train_decode in training mode
        if not isinstance(getattr(hp, "variational_dropout", False), (bool, int)):
            raise ValueError("variational_dropout=%r: True or False" % (getattr(hp, "variational_dropout"),))
        if not isinstance(getattr(hp, "lstm_layer_norm", False), (bool, int)) or getattr(hp, "lstm_layer_norm", False) not in (0, 1):
            raise ValueError("lstm_layer_norm=%r: True or False" % (getattr(hp, "lstm_layer_norm"),))
        self.pad_idx = int(hp.vocab_stoi["<PAD>"])
        # token losses: the defaults keep the label-smoothed cross entropy and its launches
        token_loss, focal_gamma, ul_alpha = getattr(hp, "token_loss", "ce"), getattr(hp, "focal_gamma", 2.0), getattr(hp, "ul_alpha", 0.0)
        criterion = TokenLoss(hp.label_smoothing, token_loss, focal_gamma, ul_alpha, self.pad_idx)      # refuses what it cannot run
        self.criterion = criterion if token_loss != "ce" or ul_alpha > 0 else LabelSmoothing(hp.label_smoothing)
        if encoder_factory is not None:                     # registered here to keep the reference's module order
            self.encoder = encoder_factory(hp)
        self.embedding = Embedding(hp.vocab_size, hp.embed_dim, max_norm=getattr(hp, "embed_norm", None), padding_idx=self.pad_idx)
        self.embedding_dropout = nn.Dropout(p=hp.embedding_dropout)
        self.init_lstm = InitLSTM(hp, bias=True)
        self.lstm = LSTM(input_size=hp.embed_dim + hp.encoder_dim, hidden_size=hp.decoder_dim, num_layers=hp.decoder_layers, bias=True)
        if getattr(hp, "lstm_layer_norm", False):           # layer-normalised cell: off, the module does not exist and the state dict is the reference's
            self.lstm_ln = LSTMLayerNorm(hp.decoder_dim, hp.decoder_layers)
        self.attention = SoftAttention(hp)
        self.beta = Gate(nn.Linear(hp.decoder_dim, hp.encoder_dim, bias=True), nn.Sigmoid())
        fan_in = self.beta[0].weight.shape[1]
        self.beta[0].bias.data.fill_(1 / fan_in)
        self.output = DeepOutput(hp)
        if hp.weight_tying and hp.deep_output:
            self.output.output.weight = self.embedding.weight

    # -- parameters in the order of sat_decoder_params (include/sat_hip.h): 18 base tensors, then 4 per stacked LSTM layer
    def param_list(self):
        o = self.output
        up = [getattr(self.lstm, "%s_l%d" % (k, l)) for l in range(1, self.hp.decoder_layers) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return [self.embedding.weight, self.init_lstm.factorize.weight, self.init_lstm.factorize.bias, self.init_lstm.init.weight,
                self.init_lstm.init.bias, self.lstm.weight_ih_l0, self.lstm.weight_hh_l0, self.lstm.bias_ih_l0, self.lstm.bias_hh_l0,
                self.attention.encoder_att.weight, self.attention.decoder_att.weight, self.attention.f_att.weight,
                self.beta[0].weight, self.beta[0].bias, o.hidden.weight, (o.context.weight if o.deep else None),
                o.output.weight, o.output.bias] + up

    def lstm_layer_norm_on(self):
        return getattr(self, "lstm_ln", None) is not None

    def ln_param_list(self):
        """the layer-norm group of the normalised cell in ``_lib.ln_param_names`` order ([] with the plain cell): it travels next to
        ``param_list()``, never inside it"""
        if not self.lstm_layer_norm_on():
            return []
        ln = self.lstm_ln
        return [getattr(getattr(ln, "%s_l%d" % (mod, l)), par) for l in range(self.hp.decoder_layers)
                for mod, par in (("gates", "weight"), ("gates", "bias"), ("cell", "weight"), ("cell", "bias"))]

    def load_decoder_state(self, sd):
        own = self.state_dict()
        for k, v in sd.items():
            if k in own:
                own[k].copy_(torch.as_tensor(v))

    # ------------------------------------------------------------------ inference (model.py:214-472)
    def _params_struct(self):
        layers = self.hp.decoder_layers
        tens = dict(zip(L.param_names(layers), self.param_list()))
        ln = dict(zip(L.ln_param_names(layers), self.ln_param_list()))
        return Dk._params_struct(tens, layers, ln), {**tens, **ln}

    @torch.no_grad()
    def beam_decode(self, ann_bld, hw, beamk=3, max_gen_length=32, temperature=1.0, sample_method="beam", sample_topk=3,
                    decoder_noise=None, rescore_method=None, rescore_reward=0.5, return_all=False, multinomial=None, randn=None,
                    topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, nucleus_log=None, no_repeat_ngram=None, min_length=None, repetition_penalty=None,
                    beam_groups=None, diversity_penalty=0.5, required=None):
        """SAT.forward's per-image beam search (model.py:260-472) on annotations (B, L, D).  The decode step,
        log-softmax / masking and top-k run in the library; the beam bookkeeping (which hypotheses to keep, finished
        lists, rescoring) stays on the host like in the reference.  ``sample_method`` "multinomial" / "topk"
        (model.py:360-379) draw the continuing hypotheses with ``multinomial(probs, k)`` and ``decoder_noise``
        (model.py:322-324) perturbs the recurrent state with ``randn(shape)``: both default to the torch samplers on the
        annotations' device and can be replaced (tests feed both sides the same draws).
        ``topg`` / ``prefix`` / ``banned`` / ``no_unk``: the constrained search ("Constrained search"), the same rules as
        ``beam_decode_batched`` with torch ops on the scores this loop already holds.
        ``sample_method="nucleus"`` with ``sample_topp``: "topk"'s draw over the top-p set of every row (``nucleus_candidates``).
        ``nucleus_log``: a list that receives, per free step, ``dict(image, step, cand, margins)`` before the draw (tests gather their
        Gumbel variates by ``cand`` and read how close every cut came to ``sample_topp``).
        ``no_repeat_ngram`` / ``min_length`` / ``repetition_penalty``: the history rules ("History rules") with torch ops
        on ``top_preds`` and the logits; the implementation ``beam_decode_batched``'s kernels are tested against."""
        import ctypes as C
        if rescore_method == "MBR":
            raise ValueError("rescore_method='MBR' (consensus reranking) runs in the batched search only (beam_decode_batched, max_gen_length >= 1)")
        if sample_method == "ancestral":
            raise ValueError("sample_method='ancestral' runs in the batched search only (beam_decode_batched, max_gen_length >= 1)")
        multinomial = multinomial or torch.multinomial
        con, hist, _, _ = constraints.SearchOptions.from_kwargs(locals()).resolve(self.hp.vocab_stoi, self.embedding.weight.shape[0], ann_bld.shape[0], beamk,
                                                                                  max_gen_length, batched=False)      # groups and required words: batched only
        lib = L.lib()
        L.require_gpu(ann_bld)
        hp = self.hp
        dev = ann_bld.device
        B, Lc, D = ann_bld.shape
        Hh, Ww = hw
        V, m = self.embedding.weight.shape
        n = self.lstm.weight_hh_l0.shape[1]
        A = self.attention.decoder_att.weight.shape[0]
        START, PAD = int(hp.vocab_stoi["<START>"]), int(hp.vocab_stoi["<PAD>"])
        END, UNK = int(hp.vocab_stoi["<END>"]), int(hp.vocab_stoi["<UNK>"])
        temps = temperature if isinstance(temperature, list) else [temperature]
        NL = int(hp.decoder_layers)
        randn = randn or (lambda shape: torch.randn(shape, device=dev))
        dims = Dk.decoder_dims(1, beamk, 2, Lc, D, A, m, n, V, 0, hp.deep_output, self.pad_idx,
                               int(getattr(self, "sat_precision", "fp32") == "bf16"), layers=NL)
        w, _keep = self._params_struct()
        ws_bytes = lib.sat_decoder_infer_workspace_bytes(C.byref(dims), beamk)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        mask_rest = torch.tensor([START, PAD], dtype=torch.int32, device=dev)
        mask_first = torch.tensor([START, PAD, END, UNK], dtype=torch.int32, device=dev)
        work = torch.empty(beamk * V, **f32)
        captions, cap_scores, cap_alphas, cap_ppl = [], [], [], []
        st = L.stream_ptr
        ban_t = torch.tensor(con.banned, dtype=torch.int64, device=dev) if con is not None and con.banned else None
        g = con.topg if con is not None else 0
        ngram, min_len = (hist.no_repeat_ngram, hist.min_length) if hist is not None else (0, 0)
        theta = torch.tensor(hist.repetition_penalty, dtype=torch.float32, device=dev) if hist is not None and hist.repetition_penalty != 1.0 else None
        for idx in range(B):
            k = beamk
            forced = con.prefix[idx] if con is not None else []       # this image's forced words; the first free step is len(forced)
            ann = ann_bld[idx].contiguous()
            h = torch.empty(NL, k, n, **f32); c = torch.empty(NL, k, n, **f32)
            L.check(lib.sat_decoder_infer_begin(C.byref(dims), C.byref(w), L.ptr(ann), k, beamk, L.ptr(h), L.ptr(c), L.ptr(ws), ws_bytes, st()),
                    "sat_decoder_infer_begin")
            top_preds = torch.full((1, k), START, dtype=torch.int64, device=dev)
            top_scores = torch.zeros(k, **f32)
            alphas = torch.zeros(1, k, Lc, **f32)
            fin_caps, fin_alphas, fin_scores, fin_ppl = [], [], [], []

            def rescore(s, step):
                if rescore_method == "LN":
                    return s / step
                if rescore_method == "WR":
                    return s + rescore_reward * step
                if rescore_method == "BAR":
                    return s + rescore_reward * (-top_scores.mean())
                return s

            step = 0
            while True:
                T = float(temps[step % len(temps)])
                tok = top_preds[step].to(torch.int32).contiguous()
                logits = torch.empty(k, V, **f32); alpha = torch.empty(k, Lc, **f32)
                noise = None
                if decoder_noise is not None and decoder_noise != 0.0:
                    noise = (randn((NL, k, n)).to(device=dev, dtype=torch.float32) * (decoder_noise / (step + 1))).contiguous()
                L.check(lib.sat_decoder_infer_step(C.byref(dims), C.byref(w), L.ptr(ann), L.ptr(tok), k, beamk, L.ptr(h), L.ptr(c), L.ptr(logits),
                                                   L.ptr(alpha), L.ptr(noise), L.ptr(ws), ws_bytes, st()), "sat_decoder_infer_step")
                said = top_preds[1:step + 1].t()            # (k, step): what every row has said, prefix words included
                if theta is not None and step > 0:          # every distinct word of the history, once: x > 0 ? x / theta : x * theta
                    seen = torch.zeros(k, V, dtype=torch.bool, device=dev).scatter_(1, said, True)
                    logits = torch.where(seen, torch.where(logits > 0, logits / theta, logits * theta), logits).contiguous()
                scores = torch.empty(k, V, **f32)
                vals = torch.empty(k, **f32); inds = torch.empty(k, dtype=torch.int32, device=dev)
                if step == 0 and not forced:
                    L.check(lib.sat_beam_scores(L.ptr(logits), k, V, T, L.ptr(mask_first), 4, None, L.ptr(scores), st()), "sat_beam_scores")
                else:
                    L.check(lib.sat_beam_scores(L.ptr(logits), k, V, T, L.ptr(mask_rest), 2, L.ptr(top_scores.contiguous()) if step else None, L.ptr(scores),
                                                st()), "sat_beam_scores")
                if ban_t is not None:
                    scores[:, ban_t] = float("-inf")
                if step >= len(forced):                 # the free steps: END waits for min_length, no n-gram is said twice
                    if step < min_len:
                        scores[:, END] = float("-inf")
                    if ngram == 1 and step > 0:
                        scores.scatter_(1, said, float("-inf"))
                    elif ngram > 1 and step >= ngram:
                        grams = said.unfold(1, ngram, 1)    # (k, step - n + 1, n): every n-gram of the history
                        hit = (grams[:, :, :ngram - 1] == said[:, step - ngram + 1:].unsqueeze(1)).all(-1)
                        rows, pos = hit.nonzero(as_tuple=True)
                        scores[rows, grams[rows, pos, ngram - 1]] = float("-inf")
                if step <= len(forced):                 # every row is its own parent up to the image's first free step
                    if step < len(forced):              # forced word: its own score joins the running sum
                        top_scores = scores[:, forced[step]].contiguous()
                        inds = torch.full((k,), forced[step], dtype=torch.int32, device=dev)
                    else:
                        L.check(lib.sat_topk(L.ptr(scores), L.ptr(work), V, k, L.ptr(vals), L.ptr(inds), st()), "sat_topk")   # row 0 only (model.py:343)
                        top_scores = vals
                    top_preds = torch.cat([top_preds, inds.to(torch.int64).unsqueeze(0)], 0)
                    alphas = torch.cat([alphas, alpha.unsqueeze(0)], 0)
                else:
                    if g:                               # top-g clipping: the g best words of every row, then the top k of the k * g candidates
                        cv, ci = torch.sort(scores, dim=1, descending=True, stable=True)
                        cv, ci = cv[:, :g].reshape(-1), (ci[:, :g] + (torch.arange(k, device=dev) * V).unsqueeze(1)).reshape(-1)
                        by_index = torch.argsort(ci)    # ties go to the lower flat index
                        top = torch.sort(cv[by_index], descending=True, stable=True).indices[:k]
                        pred, top_scores = ci[by_index][top], cv[by_index][top]
                    elif sample_method == "beam":
                        L.check(lib.sat_topk(L.ptr(scores), L.ptr(work), k * V, k, L.ptr(vals), L.ptr(inds), st()), "sat_topk")
                        top_scores = vals
                        pred = inds.to(torch.int64)
                    else:
                        if sample_method == "multinomial":                                 # model.py:360-364
                            pred = multinomial(torch.softmax(20 * scores / step, dim=1).reshape(-1), k)
                        elif sample_method == "nucleus":                                   # "topk"'s draw on the top-p set of every row
                            if nucleus_log is not None:
                                cand, margins = nucleus_candidates(scores, sample_topp, with_margin=True)
                                nucleus_log.append(dict(image=idx, step=step, cand=cand, margins=margins))
                            else:
                                cand = nucleus_candidates(scores, sample_topp)
                            choice = multinomial(torch.softmax(scores.reshape(-1)[cand] / step, dim=0), k)
                            pred = cand[choice.to(cand.device)]
                        else:                                                              # model.py:365-379
                            _, cand = torch.topk(scores, sample_topk, dim=1)
                            cand = (cand + (torch.arange(k, device=dev) * V).unsqueeze(1)).reshape(-1)
                            choice = multinomial(torch.softmax(scores.reshape(-1)[cand] / step, dim=0), k)
                            pred = cand[choice.to(cand.device)]
                        pred = pred.to(device=dev, dtype=torch.int64)
                        top_scores = scores.reshape(-1)[pred]
                    keep = torch.div(pred, V, rounding_mode="floor")
                    word = torch.remainder(pred, V).unsqueeze(0)
                    top_preds = torch.cat([top_preds[:, keep], word], 0)
                    alphas = torch.cat([alphas[:, keep], alpha.unsqueeze(0)[:, keep]], 0)
                    h, c = h[:, keep].contiguous(), c[:, keep].contiguous()
                complete = top_preds[step + 1] == END
                done = complete.tolist()
                if any(done):
                    for i, flag in enumerate(done):
                        if flag:
                            fin_caps.append(top_preds[:, i][1:-1].tolist())
                            fin_alphas.append(alphas[:, i][1:-1].reshape(-1, Hh, Ww).cpu())
                            fin_scores.append(float(rescore(top_scores[i], step)))
                            fin_ppl.append(float(torch.exp(-top_scores[i] / step)))
                    inc = ~complete
                    top_preds, alphas, top_scores = top_preds[:, inc], alphas[:, inc], top_scores[inc]
                    h, c = h[:, inc].contiguous(), c[:, inc].contiguous()
                    k = int(inc.sum())
                    if k == 0:
                        break
                if step >= max_gen_length:
                    for i in range(top_preds.shape[1]):
                        fin_caps.append(top_preds[:, i][1:-1].tolist())
                        fin_alphas.append(alphas[:, i][1:-1].reshape(-1, Hh, Ww).cpu())
                        fin_scores.append(float(rescore(top_scores[i], step)))
                        fin_ppl.append(float(torch.exp(-top_scores[i] / step)))
                    break
                step += 1
            if return_all:
                order = [i for _, i in sorted([[fin_scores[i], i] for i in range(len(fin_scores))], reverse=True)]
                captions.append([fin_caps[i] for i in order]); cap_alphas.append([fin_alphas[i] for i in order])
                cap_scores.append([fin_scores[i] for i in order]); cap_ppl.append([fin_ppl[i] for i in order])
            else:
                best = fin_scores.index(max(fin_scores))
                captions.append(fin_caps[best]); cap_alphas.append(fin_alphas[best])
                cap_scores.append(fin_scores[best]); cap_ppl.append(fin_ppl[best])
        return captions, cap_scores, cap_alphas, cap_ppl

    def _beam_search_device(self, ann_bld, beamk, max_gen_length, temperature, sample_method="beam", sample_topk=3, decoder_noise=None, seed=None, gumbel=None,
                            normals=None, graph=False, topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None,
                            min_length=None, repetition_penalty=None, beam_groups=None, diversity_penalty=0.5, required=None, options=None):
        """The device half of ``beam_decode_batched``: enqueue the whole search for annotations (B, L, D) (eagerly, or as the replay of
        its cached hipGraph) and return the buffers it leaves on the device (tok_in, prev_row, alpha_hist, fin_*: include/sat_hip.h,
        sat_beam_search_batched).  No device-to-host copy and no synchronisation (the first call of a shape with ``graph=True`` excepted).
        ``options``: a ``constraints.SearchOptions`` in place of the option keywords; ``SearchOptions.resolve`` refuses what does not
        combine, and the call is one ``sat_beam_search`` whatever the options.
        ``graph=True`` replays the "beam" search without noise, and the "nucleus" search drawn by the device generator from a
        given ``seed`` (the seed and ``sample_topp`` are arguments of the captured launches, so both are part of the cache key); a
        constraint, a history rule, groups or required words run eagerly.
        ``sample_method="ancestral"`` (``beamk == 1``, no constraint, no graph) draws every word, the first included, from the model's
        own distribution; ``gumbel`` is then (max_gen_length + 1, B, V).
        With ``required`` ("Required words") the buffers gain "req_met" (B), the most required words a finished hypothesis
        of the image contains (no such key without required words), and the fin_* lists hold the hypotheses that reach it."""
        import ctypes as C
        opt = options if options is not None else constraints.SearchOptions.from_kwargs(locals())
        con, hist, grp, req = opt.resolve(self.hp.vocab_stoi, self.embedding.weight.shape[0], ann_bld.shape[0], beamk, max_gen_length)
        L.require_gpu(ann_bld)
        hp = self.hp
        dev = ann_bld.device
        ann_bld = ann_bld.contiguous()
        B, Lc, D = ann_bld.shape
        V, m = self.embedding.weight.shape
        n = self.lstm.weight_hh_l0.shape[1]
        A = self.attention.decoder_att.weight.shape[0]
        K, S = int(beamk), int(max_gen_length)
        dims = Dk.decoder_dims(B, K, 2, Lc, D, A, m, n, V, 0, hp.deep_output, self.pad_idx, int(getattr(self, "sat_precision", "fp32") == "bf16"),
                               layers=int(hp.decoder_layers))
        w, _keep = self._params_struct()
        smp = None
        seed, gumbel, normals = opt.seed, opt.gumbel, opt.normals
        seeded = seed is not None
        if opt.sample_method != "beam" or opt.decoder_noise:
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (1,)))
            for t in (gumbel, normals):
                if t is not None:
                    L.require_gpu(t)
                    assert t.dtype == torch.float32 and t.is_contiguous()
            smp = L.BeamSampling(method=L.SAMPLE_METHODS[opt.sample_method], sample_topk=int(opt.sample_topk), seed=int(seed),
                                 gumbel=(gumbel.data_ptr() if gumbel is not None else None), decoder_noise=float(opt.decoder_noise or 0.0),
                                 sample_topp=(float(opt.sample_topp) if opt.sample_method == "nucleus" else 0.0),
                                 normals=(normals.data_ptr() if normals is not None else None))
        desc = Dk.search_desc(hp.vocab_stoi, K, S, temperature, dev, con, hist, grp, req, smp)
        desc.d, desc.w = C.pointer(dims), C.pointer(w)

        def enqueue(ann, o=None):
            desc.ann = ann.data_ptr()
            return Dk.beam_search(desc, B, Lc, dev, o)

        replayable = smp is None or (opt.sample_method == "nucleus" and seeded and gumbel is None and normals is None)
        if opt.graph and replayable and con is None and hist is None and grp is None and req is None:
            cache = self.__dict__.setdefault("_beam_graphs", {})
            temps = temperature if isinstance(temperature, list) else [temperature]
            key = (B, Lc, D, K, S, tuple(float(t) for t in temps), int(dims.precision), str(dev), tuple(t.data_ptr() for t in _keep.values() if torch.is_tensor(t)))
            if smp is not None:
                key += ("nucleus", float(smp.sample_topp), int(smp.seed), float(smp.decoder_noise))
            ent = cache.get(key)
            if ent is None:
                ann_s = ann_bld.clone()
                o = enqueue(ann_s)                      # eager once: validates the arguments and sets the kernel attributes before the capture
                torch.cuda.synchronize(dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    enqueue(ann_s, o)
                while len(cache) >= 4:                  # a few shapes at most: every entry pins its buffers
                    cache.pop(next(iter(cache)))
                ent = cache[key] = (g, ann_s, o, _keep)
            g, ann_s, o = ent[0], ent[1], ent[2]
            ann_s.copy_(ann_bld)
            g.replay()
        else:
            o = enqueue(ann_bld)
        return o

    @torch.no_grad()
    def beam_decode_batched(self, ann_bld, hw, beamk=3, max_gen_length=32, temperature=1.0, rescore_method=None, rescore_reward=0.5,
                            return_all=False, sample_method="beam", sample_topk=3, decoder_noise=None, seed=None, gumbel=None, normals=None, graph=False,
                            topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None,
                            mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0, beam_groups=None, diversity_penalty=0.5, required=None):
        """The same beam search as ``beam_decode`` ("beam" sampling, no decoder noise) for ALL images of the batch at once
        (SURVEY 8f row 2): one library call enqueues every decode step for the (B, beamk) hypothesis rows -- per-image top-k,
        completed hypotheses leaving their image's beam, cut at ``max_gen_length`` -- without a host round trip; the host reads
        the back-trace once and rebuilds the reference's four lists (model.py:449-472).
        ``sample_method`` "multinomial" / "topk" (model.py:360-379) and ``decoder_noise`` (model.py:322-324) run in the same call:
        the hypotheses are drawn on the device as the top k of log p + Gumbel noise (an ordered sample without replacement, like
        ``torch.multinomial``) from a counter-based generator seeded by ``seed`` (default: one draw from torch's CPU generator);
        ``gumbel`` / ``normals`` replace the generator by tables (layouts: include/sat_hip.h, sat_beam_sampling).
        ``graph=True`` ("beam" sampling without noise): the call's ~25 launches per decode step are captured once per (batch
        shape, beam, length, temperatures, weights) into a hipGraph over static buffers and replayed - the same kernels with the
        same arguments, one submission.
        Constraints on the selection step ("Constrained search"), all inside the same call: ``topg`` keeps only the g best
        words of every hypothesis as candidates ("beam" sampling only), ``prefix`` (token ids, or a string looked up in ``vocab_stoi``;
        one for all images or one per image) forces the first words of every caption, ``banned`` ids / ``no_unk`` never appear.
        ``graph=True`` combined with any constraint runs eagerly, as sampling does.
        ``sample_method="nucleus"`` with ``sample_topp`` in (0, 1] (top-p sampling; DESIGN.md 5, "Sampled decoding"): "topk"'s draw with
        the candidates of a hypothesis being the fewest words that carry ``sample_topp`` of its probability mass.  Prefix, banned ids
        and ``no_unk`` combine with it, ``topg`` does not; ``graph=True`` replays it when ``seed`` is given and no table is.
        ``sample_method="ancestral"`` (``beamk=1`` only; DESIGN.md 5, "Self-critical training"): pure sampling, every word drawn from
        softmax(logits / temperature) over the unmasked words, step 0 included; no constraint and no graph combine with it.
        History rules ("History rules"), in the same call and with every method but "ancestral": ``repetition_penalty``
        theta (CTRL) divides the positive and multiplies the negative raw logits of the words a hypothesis has already said,
        ``min_length`` keeps <END> masked until a caption has that many words, ``no_repeat_ngram=n`` masks every word that would say an
        n-gram of the hypothesis a second time.  Forced prefix words count as history but are obeyed.  Eager, like the constraints.
        ``rescore_method="MBR"`` ("Consensus reranking"): the finished hypotheses of an image are scored against each other
        on the device (``mbr_reward`` = the weights of CIDEr-D and ROUGE-L with the document frequencies of ``mbr_corpus``, an
        ``evaluation.ReferenceCorpus``; ``mbr_alpha`` weighs a hypothesis's vote by exp(alpha * (its raw score - the best))); the
        returned scores are the utilities, the captions come from the device back-trace, ``return_all`` orders by utility.
        ``beam_groups=G`` with ``diversity_penalty`` lambda ("Diverse beam search"): the beam is G groups of beamk / G rows,
        each a beam of its own; at a step the groups select one after the other and a group pays lambda for every hypothesis an earlier
        group kept with the same word at this step.  The penalty steers the selection only: scores stay model log-probabilities.
        "beam" sampling only; banned ids, ``no_unk``, the history rules, temperature lists and every ``rescore_method`` combine,
        ``topg`` / ``prefix`` / ``decoder_noise`` / ``graph=True`` raise ``ValueError``.  ``None``, 0 or 1: today's search.
        ``required`` ("Required words"): the words a caption must contain, one list of ids or one string of words for every
        image, or one per image (ragged; an empty one searches that image as today).  <END> is held back in a hypothesis until it has
        said them all, and the beam keeps room for the hypotheses that have said the most (dynamic beam allocation); at the end the
        finished list of an image keeps the hypotheses that contain the most required words, and every ``rescore_method`` picks among
        those.  Scores stay model log-probabilities.  "beam" sampling only; banned ids, ``no_unk``, the history rules and temperature lists
        combine, ``topg`` / ``prefix`` / ``decoder_noise`` / ``beam_groups`` / ``graph=True`` raise ``ValueError``
        (``constraints.resolve_required``).  ``None`` or empty: today's search."""
        import numpy as np
        mbr = constraints.check_mbr(rescore_method, mbr_corpus, mbr_reward, mbr_alpha, beamk, self.embedding.weight.shape[0], max_gen_length)
        o = self._beam_search_device(ann_bld, beamk, max_gen_length, temperature, options=constraints.SearchOptions.from_kwargs(locals()))
        B = ann_bld.shape[0]
        Hh, Ww = hw
        K, S = int(beamk), int(max_gen_length)
        tok_in, prev_row, alpha_hist = o["tok_in"], o["prev_row"], o["alpha_hist"]
        fin_count, fin_step, fin_row, fin_score, fin_mean = o["fin_count"], o["fin_step"], o["fin_row"], o["fin_score"], o["fin_mean"]
        if mbr is not None:                        # three launches behind the search; read with everything else below
            from . import evaluation
            hyp_tokens, hyp_len = evaluation.finished_hypotheses(o, self.pad_idx)
            utilities, _ = evaluation.consensus_utilities(hyp_tokens, hyp_len, fin_count, fin_score, mbr_corpus, mbr[:2], mbr[2])
            hyp_tokens, utilities = hyp_tokens.cpu().numpy(), utilities.cpu().numpy()
        tok_in, prev_row = tok_in.cpu().numpy(), prev_row.cpu().numpy()
        alpha_np = alpha_hist.cpu().numpy()
        fin_count, fin_step, fin_row = fin_count.cpu().numpy(), fin_step.cpu().numpy(), fin_row.cpu().numpy()
        fin_score, fin_mean = fin_score.cpu(), fin_mean.cpu()
        # back-trace of every finished hypothesis at once: walk the parent rows from the step it ended at down to step 0
        bidx = np.repeat(np.arange(B), K)[(np.arange(K)[None, :] < fin_count[:, None]).reshape(-1)]
        fidx = np.tile(np.arange(K), B)[(np.arange(K)[None, :] < fin_count[:, None]).reshape(-1)]
        hstep, cur = fin_step[bidx, fidx].astype(np.int64), fin_row[bidx, fidx].astype(np.int64)
        nh = len(bidx)
        rows = np.zeros((S + 1, nh), np.int64)
        for s_ in range(S, -1, -1):
            act = hstep >= s_
            rows[s_, act] = cur[act]
            if s_ > 0:
                cur[act] = prev_row[s_, bidx[act], cur[act]]
        sidx = np.arange(S + 1)[:, None]
        toks_all = tok_in[sidx, bidx[None, :], rows]                       # (S+1, nh): token fed at step s to the hypothesis' ancestor
        als_all = torch.from_numpy(alpha_np[sidx, bidx[None, :], rows])    # (S+1, nh, L)
        if rescore_method == "LN":
            resc = fin_score[bidx, fidx] / torch.from_numpy(hstep).float()
        elif rescore_method == "WR":
            resc = fin_score[bidx, fidx] + rescore_reward * torch.from_numpy(hstep).float()
        elif rescore_method == "BAR":
            resc = fin_score[bidx, fidx] + rescore_reward * (-fin_mean[bidx, fidx])
        elif mbr is not None:
            resc = torch.from_numpy(utilities[bidx, fidx])
        else:
            resc = fin_score[bidx, fidx]
        ppl_all = torch.exp(-fin_score[bidx, fidx] / torch.from_numpy(hstep).float())
        resc, ppl_all = resc.tolist(), ppl_all.tolist()
        captions, cap_scores, cap_alphas, cap_ppl = [], [], [], []
        hpos = 0
        for b in range(B):
            fin_caps, fin_alphas, fin_scores, fin_ppl = [], [], [], []
            for f in range(int(fin_count[b])):
                hh, step = hpos + f, int(hstep[hpos + f])
                # top_preds[:, i][1:-1] / alphas[:, i][1:-1] (model.py:412-413): without START / the zero map and without the last step
                fin_caps.append(toks_all[1:step + 1, hh].tolist() if mbr is None else hyp_tokens[b, f, :step].tolist())
                fin_alphas.append(als_all[:step, hh].reshape(-1, Hh, Ww).clone())
                fin_scores.append(resc[hh]); fin_ppl.append(ppl_all[hh])
            hpos += int(fin_count[b])
            if return_all:
                order = [i for _, i in sorted([[fin_scores[i], i] for i in range(len(fin_scores))], reverse=True)]
                if mbr is not None:                # utility descending, append order among equals
                    order = sorted(range(len(fin_scores)), key=lambda i: -fin_scores[i])
                captions.append([fin_caps[i] for i in order]); cap_alphas.append([fin_alphas[i] for i in order])
                cap_scores.append([fin_scores[i] for i in order]); cap_ppl.append([fin_ppl[i] for i in order])
            else:
                best = fin_scores.index(max(fin_scores))
                captions.append(fin_caps[best]); cap_alphas.append(fin_alphas[best])
                cap_scores.append(fin_scores[best]); cap_ppl.append(fin_ppl[best])
        return captions, cap_scores, cap_alphas, cap_ppl

    def weight_drop_args(self):
        """(weight_drop, variational_dropout) as hyper-parameters; like nn.Dropout they act in training mode only"""
        return float(getattr(self.hp, "weight_drop", 0.0)), bool(getattr(self.hp, "variational_dropout", False))

    def _dropout_args(self, seed=None):
        """(p, p_embedding, seed) of this call, or (p, p_embedding, seed, weight_drop, variational_dropout) when one of the last two is
        on: nn.Dropout is the identity in eval mode, and so are they; the seed comes from a generator of its own so that the CPU generator
        stream of scheduled sampling (F7) stays exactly the reference's."""
        p, pe = float(self.hp.dropout), float(self.hp.embedding_dropout)
        wd, var = self.weight_drop_args()
        var = var and (p > 0.0 or pe > 0.0)                 # locks the masks of those two rates: nothing to lock without them
        if not self.training or (p == 0.0 and pe == 0.0 and wd == 0.0):
            return (0.0, 0.0, 0)
        if seed is None:
            gen = self.__dict__.get("_dropout_gen")
            if gen is None:
                gen = self.__dict__["_dropout_gen"] = torch.Generator().manual_seed(torch.initial_seed() & 0x7FFFFFFFFFFFFFFF)
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=gen))
        if wd == 0.0 and not var:
            return (p, pe, int(seed))
        return (p, pe, int(seed), wd, var)

    def reg_coefficients(self):
        """(ar_alpha, tar_beta) of the activation regularisers; (0, 0): off, the step issues no launch for them"""
        return float(getattr(self.hp, "ar_alpha", 0.0)), float(getattr(self.hp, "tar_beta", 0.0))

    def add_reg_terms(self, loss, reg):
        """loss + ar_alpha * ar + tar_beta * tar from the device pair ``reg``; a coefficient of zero adds no term"""
        ar_alpha, tar_beta = self.reg_coefficients()
        if ar_alpha:
            loss = loss + ar_alpha * reg[0]
        if tar_beta:
            loss = loss + tar_beta * reg[1]
        return loss

    def token_loss_on(self):
        """the criterion is ``TokenLoss`` (``token_loss`` other than "ce", or ``ul_alpha`` > 0)"""
        return isinstance(self.criterion, TokenLoss)

    def token_loss_key(self):
        """(token_loss, focal_gamma, ul_alpha) as the criterion runs them: what a captured step depends on"""
        c = self.criterion
        return (c.token_loss, c.focal_gamma, c.ul_alpha) if self.token_loss_on() else ("ce", 0.0, 0.0)

    def token_criterion(self, logits_packed, targets_packed, caps_i32, plan):
        """the criterion on packed rows; ``TokenLoss`` also gets the ground-truth captions and the plan its candidates come from"""
        if self.token_loss_on():
            return self.criterion(logits_packed, targets_packed, (caps_i32, plan))
        return self.criterion(logits_packed, targets_packed)

    def attention_term(self, alphas):
        """the doubly-stochastic attention term ``att_gamma * ((1 - alphas.sum(dim=1)) ** 2).mean()`` (model.py:594) of a loss built on
        ``train_decode(with_loss=False)``: ``scst.loss`` and ``distill.loss`` add it to their own criterion"""
        return Dk.DoublyStochasticFn.apply(alphas, float(self.hp.att_gamma))

    def train_decode(self, ann_bld, caps, lengths, epsilon=0, draw=None, with_loss=True, dropout_seed=None, teacher=None, leaf_side=False, with_reg=None):
        """Decoder half of train_batch + the loss terms (model.py:487-557, 592-597).

        ann_bld (B, L, D) on the GPU; caps (B, R, T) int64; lengths (B, R) int64 (host or device).  ``teacher``: the scheduled-sampling
        decisions of this batch when the caller has drawn them already (``PackPlan.teacher_flags``; graph.py keys its graphs by them).
        ``leaf_side``: ``ann_bld`` comes from an encoder whose backward forks to the side stream (``encoder.decoder_leaf_side_for``).
        ``with_reg``: also return ``reg``, the device pair (ar, tar) of the top-layer states, differentiable; by default with the loss
        terms when ``ar_alpha`` or ``tar_beta`` is set, and then ``ar`` / ``tar`` (detached) come with them.  With ``TokenLoss`` as the
        criterion ``ce`` is the whole token loss and ``token_terms`` its unweighted parts; without the loss terms ``caps_i32`` comes back
        for the caller's criterion."""
        B, R, T = caps.shape
        if with_reg is None:
            with_reg = bool(with_loss) and any(self.reg_coefficients())
        plan = Dk.PackPlan.cached(lengths.reshape(-1).cpu(), T, ann_bld.device)
        if teacher is None:
            teacher = plan.teacher_flags(float(epsilon), draw)
        caps2 = caps.reshape(B * R, T)
        caps_i32 = caps2.to(device=ann_bld.device, dtype=torch.int32).contiguous()
        ln = self.ln_param_list()
        if ln:              # the normalised cell: the same call with the layer-norm group behind the parameter list
            fn = Dk.DecoderTrainLNRegFn if with_reg else Dk.DecoderTrainLNFn
        else:
            fn = Dk.DecoderTrainRegFn if with_reg else Dk.DecoderTrainFn
        logits_packed, alphas, *reg = fn.apply(ann_bld, caps_i32, plan, teacher, bool(self.hp.deep_output), self.pad_idx, R,
                                               int(getattr(self, "sat_precision", "fp32") == "bf16"), getattr(self.hp, "embed_norm", None) or 0.0,
                                               self._dropout_args(dropout_seed), bool(leaf_side), *([len(ln)] if ln else []), *self.param_list(), *ln)
        targets_packed = plan.pack(caps2[:, 1:].to(ann_bld.device).unsqueeze(-1)).squeeze(-1)
        extra = dict(reg=reg[0]) if with_reg else {}
        if not with_loss:
            return dict(logits_packed=logits_packed, targets_packed=targets_packed, alphas=alphas, plan=plan, caps_i32=caps_i32, **extra)
        ce = self.token_criterion(logits_packed, targets_packed, caps_i32, plan)
        if self.token_loss_on():
            extra.update(token_terms=self.criterion.last_terms)
        ds = Dk.DoublyStochasticFn.apply(alphas, float(self.hp.att_gamma))
        if with_reg:
            extra.update(ar=reg[0][0].detach(), tar=reg[0][1].detach())
        return dict(logits_packed=logits_packed, targets_packed=targets_packed, alphas=alphas, ce=ce, ds=ds,
                    acc=self.criterion.last_accuracy, plan=plan, **extra)


class SAT(SATDecoder, _Base):
    """``class SAT(pl.LightningModule)`` of the reference (model.py:134-199) for the train-step hot path.

    Same constructor kwargs (train.py:264 passes ``**vars(args)``), same sub-module attribute names and
    state-dict keys; ``train_batch`` / ``training_step`` / ``configure_optimizers`` keep their signatures.
    Construction order follows the reference (criterion, encoder, embedding, init_lstm, lstm, attention, beta,
    output) so that a seed produces the same parameter stream.  ``caption`` / ``forward`` run the reference's per-image
    beam search (beam / multinomial / topk sampling, decoder noise) on the HIP step kernels; ``score_captions`` / ``val_batch`` /
    ``validation_step`` (model.py:646-718) use metrics.py, the nltk algorithms restated."""

    def __init__(self, **kwargs):
        nn.Module.__init__(self)
        hp = _HParams(kwargs)
        for k, v in dict(encoder_size=None, embed_norm=None, pretrained_embedding=None, pretrained=False, decoder_tf=None,
                         decoder_tf_min=0.5, epochs=10, encoder_finetune_after=-1, att_gamma=1.0, label_smoothing=0.0,
                         dropout=0.0, embedding_dropout=0.0, weight_tying=False, deep_output=False, decoder_layers=1,
                         lr_warmup_steps=0, ar_alpha=0.0, tar_beta=0.0, token_loss="ce", focal_gamma=2.0, ul_alpha=0.0,
                         weight_drop=0.0, variational_dropout=False, lstm_layer_norm=False).items():
            hp.setdefault(k, v)
        self.scheduler = None
        self.opt_init_lr = None
        self.__dict__["_sat_global_step"] = 0           # optimizer steps taken (Lightning's trainer.global_step when no trainer is attached)
        self.__dict__["_sat_micro_batches"] = 0         # training_step calls inside the current accumulation window
        # reference order: criterion -> encoder -> decoder parts (model.py:148-195); get_encoder writes
        # hp.encoder_dim back when no projection is needed (model.py:56)
        self._build_decoder(hp, encoder_factory=get_encoder)
        # train.py:31-32 `--precision 16` asks Lightning for torch AMP (fp16 autocast + GradScaler).  The MI355X-native reduced-precision mode is
        # bf16 storage / bf16 MFMA with fp32 accumulation, master weights and losses (fp32 exponent range: no loss scaling needed); there is no
        # fp16 path.  `hip_precision` overrides.
        amp = str(hp.get("precision", 32)) in ("16", "bf16", "16-mixed", "bf16-mixed")
        self.set_precision(hp.get("hip_precision", "bf16" if amp else "fp32"))
        if hp.pretrained_embedding is not None:
            import numpy as np
            self.embedding.weight = nn.Parameter(torch.tensor(np.load(hp.pretrained_embedding), dtype=torch.float32))
        self.special_idxs = [self.stoi("<PAD>"), self.stoi("<START>"), self.stoi("<END>")]

    def set_precision(self, mode):
        """"fp32": exact fp32 MFMA everywhere (parity mode).  "bf16": bf16 matrix cores with fp32 accumulation --
        bf16 activations/filter copies in the encoder, fp32 decoder state rounded on the way into LDS; master
        weights, gradients of parameters, statistics and losses stay fp32."""
        if mode not in ("fp32", "bf16"):
            raise ValueError("hip_precision must be 'fp32' or 'bf16'")
        self.sat_precision = mode
        self.encoder.precision = mode

    # Lightning gives `hparams`; without Lightning keep the same attribute
    @property
    def hparams(self):
        return self.hp

    def stoi(self, s):
        return int(self.hp.vocab_stoi.get(s, self.hp.vocab_stoi["<UNK>"]))

    def itos(self, i):
        return str(self.hp.vocab_itos.get(int(i), "<UNK>"))

    def decode_seq(self, seq, remove_special=False):
        return [str(self.itos(t)) for t in seq if not (remove_special and t in self.special_idxs)]

    # ------------------------------------------------------------------ train_batch (model.py:474-557)
    def encode(self, img):
        ann = self.encoder(img)                                  # (B, D, h, w), channels-last memory
        B, D, h, w = ann.shape
        return ann.permute(0, 2, 3, 1).reshape(B, h * w, D), (h, w)

    @torch.no_grad()
    def caption(self, img_tensor, beamk=3, max_gen_length=32, temperature=1.0, sample_method="beam", sample_topk=3,
                decoder_noise=None, rescore_method=None, rescore_reward=0.5, return_all=False, topg=None, prefix=None, banned=None, no_unk=False,
                sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None, mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0,
                beam_groups=None, diversity_penalty=0.5, required=None):
        """model.py:214-235: eval mode, then forward.  ``topg`` / ``prefix`` / ``banned`` / ``no_unk`` / ``sample_topp``, the history
        rules ``no_repeat_ngram`` / ``min_length`` / ``repetition_penalty`` and ``rescore_method="MBR"`` with ``mbr_corpus`` /
        ``mbr_reward`` / ``mbr_alpha``, and the diverse beam search ``beam_groups`` / ``diversity_penalty``: ``beam_decode_batched``."""
        self.eval()
        opt = constraints.SearchOptions.from_kwargs(locals())
        return self.forward(img_tensor, beamk=beamk, max_gen_length=max_gen_length, temperature=temperature, rescore_method=rescore_method,
                            rescore_reward=rescore_reward, return_all=return_all, mbr_corpus=mbr_corpus, mbr_reward=mbr_reward, mbr_alpha=mbr_alpha,
                            **opt.kwargs(SAT.forward))

    def forward(self, img, beamk=3, max_gen_length=32, temperature=1.0, sample_method="beam", sample_topk=3, decoder_noise=None,
                rescore_method=None, rescore_reward=0.5, return_all=False, topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None,
                mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0, beam_groups=None, diversity_penalty=0.5, required=None):
        """Inference only (model.py:237-472): encode the batch once, then beam-search every image."""
        opt = constraints.SearchOptions.from_kwargs(locals(), graph=bool(self.__dict__.get("beam_graph", False)))      # model.beam_graph = True: hipGraph replay
        opt.resolve(self.hp.vocab_stoi, self.hp.vocab_size, img.shape[0], beamk, max_gen_length, batched=max_gen_length >= 1)        # refuse before any launch
        if sample_method == "ancestral" and max_gen_length < 1:
            raise ValueError("sample_method='ancestral' runs in the batched search only (max_gen_length >= 1)")
        constraints.check_mbr(rescore_method, mbr_corpus, mbr_reward, mbr_alpha, beamk, self.hp.vocab_size, max_gen_length)
        with torch.no_grad():
            ann_bld, hw = self.encode(img)
            if max_gen_length >= 1:        # every image at once; sampled continuations and decoder noise draw from the device generator
                return self.beam_decode_batched(ann_bld.contiguous(), hw, beamk=beamk, max_gen_length=max_gen_length, temperature=temperature,
                                                rescore_method=rescore_method, rescore_reward=rescore_reward, return_all=return_all, mbr_corpus=mbr_corpus,
                                                mbr_reward=mbr_reward, mbr_alpha=mbr_alpha, **opt.kwargs(SATDecoder.beam_decode_batched))
            return self.beam_decode(ann_bld.contiguous(), hw, beamk=beamk, max_gen_length=max_gen_length, temperature=temperature, rescore_method=rescore_method,
                                    rescore_reward=rescore_reward, return_all=return_all, **opt.kwargs(SATDecoder.beam_decode))

    def train_batch(self, batch, epsilon=0, draw=None, teacher=None):
        img, encoded_captions, lengths = batch
        ann_bld, _ = self.encode(img)
        res = self.train_decode(ann_bld, encoded_captions, lengths, float(epsilon), draw, with_loss=False, teacher=teacher,
                                leaf_side=E.decoder_leaf_side_for(self.encoder, img))
        plan = res["plan"]
        lp = PackedSequence(res["logits_packed"], plan.batch_sizes, plan.sorted_indices_dev, plan.unsorted_indices_dev)
        tp = PackedSequence(res["targets_packed"], plan.batch_sizes, plan.sorted_indices_dev, plan.unsorted_indices_dev)
        return lp, tp, res["alphas"]

    def calibrate_temperature(self, batches, max_batches=42, **fit_kwargs):
        """The reference's temperature_scaling.py in one call: teacher-forced logits of the frozen model over ``batches``, then the
        temperature fit (calibration.py).  Returns a ``TemperatureFit``; its ``temperature`` is what ``caption`` / ``val_batch`` take.
        Changes no parameter, buffer or hyper-parameter.  The fit minimises the plain negative log-likelihood: ``token_loss`` /
        ``focal_gamma`` / ``ul_alpha`` are not applied here."""
        from . import calibration
        return calibration.calibrate_temperature(self, batches, max_batches, **fit_kwargs)

    def teacher_forcing_epsilon(self, current_epoch=0):
        """model.py:565-582 (host scalars)."""
        hp = self.hp
        if hp.decoder_tf is None:
            return 0.0
        if hp.decoder_tf == "always":
            return 1.0
        if hp.decoder_tf == "linear":
            return 1 - (1 - hp.decoder_tf_min) * current_epoch / hp.epochs
        if hp.decoder_tf == "inv_sigmoid":
            l = -math.log(hp.decoder_tf_min / (1 - hp.decoder_tf_min)); g = 5.0
            b = (1 / ((l / g) + 1)) * hp.epochs
            return 1 / (1 + math.exp((g / b) * (current_epoch - b)))
        if hp.decoder_tf == "exp":
            return math.exp(math.log(hp.decoder_tf_min) / hp.epochs) ** current_epoch
        raise ValueError("decoder_tf=%r" % (hp.decoder_tf,))

    def sat_global_step(self):
        """Lightning's ``trainer.global_step`` (optimizer steps taken so far); without a trainer, the module's own count:
        one more every ``hparams.accumulate`` calls of ``training_step`` (train.py:70-71, 267)."""
        tr = getattr(self, "_trainer", None) if pl is not None else None
        if tr is not None:
            return int(tr.global_step)
        return int(self.__dict__["_sat_global_step"])

    def _train_optimizer(self):
        """the optimizer ``configure_optimizers`` built: Lightning's ``self.optimizers()`` under a trainer"""
        if pl is not None and getattr(self, "_trainer", None) is not None:
            return self.optimizers()
        return self.__dict__.get("_sat_optimizer")

    def averaged_weights(self):
        """``with model.averaged_weights():`` evaluate, caption or save with the averaged weights (``opt="asgd"`` / ``ema_decay``) in the
        parameters: ``FusedOptimizer.averaged_weights`` of the optimizer ``configure_optimizers`` built.  BatchNorm's running statistics are
        not averaged."""
        opt = self._train_optimizer()
        if not hasattr(opt, "averaged_weights"):
            raise RuntimeError("averaged_weights: configure_optimizers has not built a FusedOptimizer")
        return opt.averaged_weights()

    def step_learning_rate(self, gstep):
        """model.py:614-626, run at the end of every ``training_step`` with the optimizer steps taken so far: linear warm-up of
        every group's LR from ``opt_init_lr`` while ``gstep < lr_warmup_steps``; afterwards the per-batch schedulers
        (CosineAnnealingWarmRestarts, OneCycleLR) advance once per call."""
        hp = self.hp
        opt = self._train_optimizer()
        if opt is None or self.opt_init_lr is None:          # the caller drives its own optimizer (configure_optimizers never ran)
            return
        if gstep < hp.lr_warmup_steps:
            lr_scale = min(1, float(gstep + 1) / hp.lr_warmup_steps)
            for pg, init_lr in zip(opt.param_groups, self.opt_init_lr):
                pg["lr"] = lr_scale * init_lr
        elif gstep > 0:
            if type(self.scheduler) in [CosineAnnealingWarmRestarts, OneCycleLR]:
                self.scheduler.step()

    def _step_begin(self):
        """host half of ``training_step`` in front of the device work (model.py:559-586): (epsilon, optimizer steps so far); unfreezes the
        encoder at ``encoder_finetune_after``"""
        hp = self.hp
        epoch = int(getattr(self, "current_epoch", 0) or 0)        # Lightning's property, or a plain attribute set by the caller's loop
        epsilon = self.teacher_forcing_epsilon(epoch)
        gstep = self.sat_global_step()
        if gstep == hp.encoder_finetune_after and hp.encoder_finetune_after >= 0:
            for p in self.encoder.parameters():
                p.requires_grad = True
        return epsilon, gstep

    def _step_losses(self, batch, epsilon, teacher=None):
        """device half: forward + the two loss terms (model.py:588-597); with ``ar_alpha`` / ``tar_beta`` set, plus the activation
        regularisers, whose unweighted values it leaves in ``_sat_last_reg`` for the metrics; with ``TokenLoss`` as the criterion the
        token loss gets the ground-truth captions and the plan (whatever word was fed back, the candidates come from the references)"""
        if not any(self.reg_coefficients()) and not self.token_loss_on():
            self.__dict__["_sat_last_reg"] = None
            lp, tp, alphas = self.train_batch(batch, epsilon, teacher=teacher)
            loss = self.criterion(lp.data, tp.data)                                   # model.py:592
            loss = loss + Dk.DoublyStochasticFn.apply(alphas, float(self.hp.att_gamma))      # model.py:594
            return loss
        img, encoded_captions, lengths = batch                                    # train_batch, keeping the third output of the decoder
        ann_bld, _ = self.encode(img)
        res = self.train_decode(ann_bld, encoded_captions, lengths, float(epsilon), None, with_loss=False, teacher=teacher,
                                leaf_side=E.decoder_leaf_side_for(self.encoder, img), with_reg=any(self.reg_coefficients()))
        loss = self.token_criterion(res["logits_packed"], res["targets_packed"], res["caps_i32"], res["plan"])
        loss = loss + Dk.DoublyStochasticFn.apply(res["alphas"], float(self.hp.att_gamma))
        if "reg" not in res:
            self.__dict__["_sat_last_reg"] = None
            return loss
        self.__dict__["_sat_last_reg"] = (res["reg"][0].detach(), res["reg"][1].detach())
        return self.add_reg_terms(loss, res["reg"])

    def _reg_metrics(self):
        """{"ar", "tar"}: the unweighted regularisers of the last ``_step_losses`` (device scalars), or nothing when they are off; with
        ``TokenLoss`` as the criterion also {"ce", "fl", "ul", "repeat_mass"}, the unweighted parts of the token loss"""
        reg = self.__dict__.get("_sat_last_reg")
        out = {} if reg is None else {"ar": reg[0], "tar": reg[1]}
        if self.token_loss_on():
            out.update(self.criterion.last_terms)
        return out

    def _step_end(self, gstep):
        """host half behind the device work (model.py:614-626): learning-rate recipe, optimizer-step count"""
        hp = self.hp
        self.step_learning_rate(gstep)                                            # model.py:614-626
        micro = self.__dict__["_sat_micro_batches"] + 1
        if micro >= max(1, int(getattr(hp, "accumulate", 1) or 1)):                # the trainer steps the optimizer after this batch
            self.__dict__["_sat_global_step"] += 1
            micro = 0
        self.__dict__["_sat_micro_batches"] = micro

    def training_step(self, batch, batch_idx=0):
        """model.py:559-628: returns the metrics dict whose "loss" the trainer back-propagates.  (Split in three so that
        ``graph.GraphedTrainStep`` can replay the device half from a hipGraph and still run the two host halves every step.)
        With ``ar_alpha`` / ``tar_beta`` set (Merity et al.'s activation regularisers on the top-layer LSTM states) the loss gains
        ``ar_alpha * ar + tar_beta * tar`` and the dict ``"ar"`` and ``"tar"``, the unweighted device scalars.  With ``token_loss`` in
        "fl" / "ce+fl" or ``ul_alpha`` > 0 ("Token losses") the cross entropy gives way to ``TokenLoss`` and the dict gains
        ``"ce"``, ``"fl"``, ``"ul"`` and ``"repeat_mass"``, again unweighted device scalars."""
        epsilon, gstep = self._step_begin()
        loss = self._step_losses(batch, epsilon)
        self._step_end(gstep)
        return {"loss": loss, "accuracy": self.criterion.last_accuracy, "epsilon_tf": float(epsilon), **self._reg_metrics()}

    def scst_step(self, batch, corpus, samples=5, baseline="mean", reward=(1.0, 0.0), max_gen_length=20, temperature=1.0, seed=None):
        """Self-critical sequence training (Rennie et al. 2017; DESIGN.md 5, "Self-critical training"): the counterpart of
        ``training_step`` for the second training stage, ``scst.step`` with this module's two host halves around it.  ``batch`` is
        ``training_step``'s (img, references (B, R, T), lengths (B, R)); ``corpus`` a ``ReferenceCorpus`` holding the split's document
        frequencies.  Returns ``{"loss", "reward", "baseline_reward", "advantage_abs", "sample_length"}`` (device scalars: the loss the
        trainer back-propagates, and batch means) plus ``"samples"`` / ``"sample_lengths"`` / ``"rewards"`` / ``"advantages"``, the
        device tensors they were taken from.  ``ar_alpha`` / ``tar_beta`` are not applied here: the activation regularisers belong to
        ``training_step``'s loss alone, and so do ``token_loss`` / ``focal_gamma`` / ``ul_alpha``."""
        from . import scst
        scst.check_step_args(self, corpus, samples, baseline, reward, max_gen_length, temperature)        # refuse before any launch
        _, gstep = self._step_begin()
        out = scst.step(self, batch, corpus, samples, baseline, reward, max_gen_length, temperature, seed)
        self._step_end(gstep)
        return out

    def distill_step(self, batch, teacher, alpha=0.5, temperature=2.0, targets="references", beamk=3, max_gen_length=20):
        """Knowledge distillation (Hinton et al. 2015; DESIGN.md 5, "Distillation"): the counterpart of ``training_step`` with a teacher,
        ``distill.step`` with this module's two host halves around it.  ``teacher``: another ``SAT`` or an ``Ensemble``; ``batch`` is
        ``training_step``'s.  ``targets="teacher"`` trains on the teacher's best beam caption (``beamk``, ``max_gen_length``) in place of
        the references.  Returns ``{"loss", "hard", "soft", "accuracy"}`` (device scalars: the loss the trainer back-propagates, the
        label-smoothed cross entropy, the KL to the teacher and the next-word accuracy).  ``ar_alpha`` / ``tar_beta`` are not applied
        here: the activation regularisers belong to ``training_step``'s loss alone, and so do ``token_loss`` / ``focal_gamma`` /
        ``ul_alpha`` (the hard term stays the label-smoothed cross entropy)."""
        from . import distill
        distill.check_step_args(self, teacher, alpha, temperature, targets, beamk, max_gen_length)        # refuse before any launch
        _, gstep = self._step_begin()
        out = distill.step(self, batch, teacher, alpha, temperature, targets, beamk, max_gen_length)
        self._step_end(gstep)
        return out

    # ------------------------------------------------------------------ validation (model.py:630-718)
    def _log_scalar(self, key, val, step):
        """tensorboard scalar when a Lightning-style logger is attached (model.py:611, 635, 708); a no-op otherwise"""
        logger = getattr(self, "logger", None)
        exp = getattr(logger, "experiment", None)
        if exp is not None and hasattr(exp, "add_scalar"):
            exp.add_scalar(key, val, global_step=step)

    def training_epoch_end(self, outputs):
        """model.py:630-644: epoch means of the step metrics, learning rate, per-epoch scheduler step."""
        epoch = int(getattr(self, "current_epoch", 0))
        means = {}
        for k in outputs[0].keys():
            vals = [float(x[k]) for x in outputs]
            means[k] = sum(vals) / len(vals) if vals else 0
            self._log_scalar("{}/train_epoch".format(k), means[k], epoch + 1)
        if isinstance(getattr(self, "scheduler", None), (MultiStepLR, ExponentialLR)):
            self.scheduler.step()
        return means

    @torch.no_grad()
    def score_captions(self, captions, encoded_captions, lengths, perplexities=None):
        """model.py:646-682: corpus BLEU-1..4 and GLEU of the generated captions against the R references of each image, and the
        best cosine similarity between mean embeddings.  BLEU / GLEU: metrics.py (nltk's algorithms restated; nltk is a host-side
        dependency of the reference and runs on token-id lists); the embedding part runs on the device."""
        from . import metrics
        lens = lengths.tolist() if torch.is_tensor(lengths) else lengths
        references = [[c[1:l] for c, l in zip(refs, lens[i])] for i, refs in enumerate(encoded_captions.tolist())]
        out = {"bleu1": metrics.corpus_bleu(references, captions, weights=(1, 0, 0, 0)),
               "bleu2": metrics.corpus_bleu(references, captions, weights=(0.5, 0.5, 0, 0)),
               "bleu3": metrics.corpus_bleu(references, captions, weights=(0.33, 0.33, 0.33, 0)),
               "bleu4": metrics.corpus_bleu(references, captions, weights=(0.25, 0.25, 0.25, 0.25))}
        dev = self.embedding.weight.device
        enc = encoded_captions.to(dev)
        E = self.embedding.weight
        cossims = torch.zeros(enc.shape[0], dtype=torch.float, device=dev)
        for i in range(enc.shape[0]):
            cv = E[torch.as_tensor(captions[i], dtype=torch.long, device=dev)].mean(0).unsqueeze(0)
            rvs = torch.zeros(enc.shape[1], dtype=torch.float, device=dev)
            for j, l in enumerate(lens[i]):
                rv = E[enc[i][j][1:l]].mean(0).unsqueeze(0)
                rvs[j] = F.cosine_similarity(rv, cv)
            cossims[i] = rvs.max()
        out["cosine_similarity"] = cossims.mean().item()
        out["gleu"] = metrics.corpus_gleu(references, captions)
        if type(perplexities) == list:
            out["perplexity"] = sum(perplexities) / len(perplexities)
        return out

    def val_batch(self, batch, beamk=3, max_gen_length=32, temperature=0.5, sample_method="beam", sample_topk=3, decoder_noise=None,
                  rescore_method=None, rescore_reward=0.5, topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None,
                  beam_groups=None, diversity_penalty=0.5, required=None):
        """model.py:684-691"""
        kw = _named(locals())
        img, encoded_captions, lengths = kw.pop("batch")
        captions, scores, alphas, perplexities = self.caption(img, return_all=False, **kw)
        return self.score_captions(captions, encoded_captions, lengths, perplexities)

    def caption_tokens(self, img, beamk=3, max_gen_length=32, temperature=1.0, sample_method="beam", sample_topk=3, decoder_noise=None,
                       rescore_method=None, rescore_reward=0.5, seed=None, graph=False, topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None,
                       mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0, corpus=None, beam_groups=None, diversity_penalty=0.5, required=None):
        """``caption(..., return_all=False)`` left on the device: (tokens, lengths, scores, perplexities), no host round trip (evaluation.py)"""
        kw = _named(locals())
        from . import evaluation
        return evaluation.caption_tokens(self, **kw)

    def val_batch_stats(self, batch, beamk=3, max_gen_length=32, temperature=0.5, sample_method="beam", sample_topk=3, decoder_noise=None,
                        rescore_method=None, rescore_reward=0.5, seed=None, graph=False, corpus=None, topg=None, prefix=None, banned=None, no_unk=False,
                        sample_topp=0.9, chrf=None, chrf_beta=3.0, no_repeat_ngram=None, min_length=None, repetition_penalty=None, mbr_corpus=None,
                        mbr_reward=(1.0, 0.0), mbr_alpha=0.0, beam_groups=None, diversity_penalty=0.5, required=None, with_diversity=False):
        """``val_batch`` as an ``evaluation.CaptionStats``: the batch is scored on the device; ``.metrics()`` gives ``val_batch``'s dict
        (with ``corpus``, an ``evaluation.ReferenceCorpus``, also CIDEr-D and ROUGE-L; with ``chrf``, an ``evaluation.VocabChars``, also chrF;
        ``with_diversity``: ``.diversity``, an ``evaluation.DiversityStats`` over every finished hypothesis of the batch)"""
        kw = _named(locals())
        from . import evaluation
        return evaluation.val_batch_stats(self, **kw)

    def visualize(self, items, beamk=3, max_gen_length=32, temperature=1.0, sample_method="beam", sample_topk=3, decoder_noise=None,
                  rescore_method=None, rescore_reward=1.0, visual_size=256, input_size=None, topg=None, prefix=None, banned=None, no_unk=False,
                  sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None, mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0,
                  beam_groups=None, diversity_penalty=0.5, required=None, **render):
        """visualize.ipynb's ``make_visual`` for a batch of picture files / bytes / arrays: load_square -> prepare_image -> search -> the
        attention overlays of every winning caption, rendered on the device.  Returns a ``visualize.Visual`` (visualize.py).
        ``progressive=True`` among ``render``: progressive JPEG files are decoded on the GPU too"""
        kw = _named(locals())
        render = kw.pop("render")
        from . import visualize
        return visualize.visualize(self, **kw, **render)

    def caption_image(self, items, beamk=3, max_gen_length=32, temperature=1.0, sample_method="beam", sample_topk=3, decoder_noise=None,
                      rescore_method=None, rescore_reward=1.0, visual_size=256, input_size=None, seed=None, progressive=False,
                      topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None,
                      mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0, beam_groups=None, diversity_penalty=0.5, required=None):
        """``caption(prepare_image(load_square(path, visual_size), input_size))`` for a batch: (captions, words, scores, perplexities).
        ``progressive``: progressive JPEG files are decoded on the GPU too (``jpeg.parse(progressive=True)``)"""
        kw = _named(locals())
        from . import visualize
        return visualize.caption_image(self, **kw)

    def validation_step(self, batch, batch_idx=0):
        """model.py:693-697"""
        return self.val_batch(batch, beamk=self.hp.val_beamk, max_gen_length=self.hp.val_max_len, temperature=1.0, rescore_method="LN")

    def validation_epoch_end(self, outputs):
        """model.py:699-718: epoch means; the monitored ones go to ``self.log`` when a trainer is attached; plateau scheduler step."""
        epoch = int(getattr(self, "current_epoch", 0))
        means, plateau_val = {}, None
        for k in outputs[0].keys():
            vals = [x[k] for x in outputs]
            try:
                val = sum(vals) / len(vals)
            except Exception:
                val = 0
            means[k] = val
            if epoch != 0:
                self._log_scalar("{}/val_epoch".format(k), val, epoch + 1)
            if hasattr(self, "log") and getattr(self, "_trainer", None) is not None and k in (getattr(self.hp, "save_monitor", None), getattr(self.hp, "early_stop_monitor", None)):
                self.log(k, val)
            if k == getattr(self.hp, "plateau_monitor", None):
                plateau_val = val
        if isinstance(getattr(self, "scheduler", None), ReduceLROnPlateau) and plateau_val is not None:
            self.scheduler.step(plateau_val)
        return means

    # ------------------------------------------------------------------ configure_optimizers (model.py:720-817)
    def configure_optimizers(self):
        hp = self.hp

        def groups(modules, weight_decay, lr):
            decay, no_decay = [], []
            for mod in modules:
                for _, p in mod.named_parameters():
                    if p.requires_grad:
                        (no_decay if p.dim() == 1 else decay).append(p)
            return [{"params": no_decay, "lr": lr, "weight_decay": 0.0}, {"params": decay, "lr": lr, "weight_decay": weight_decay}]

        dec = [self.init_lstm, self.lstm, self.attention, self.beta, self.output]
        if self.lstm_layer_norm_on():                       # gains and shifts are 1-D: the decoder's no-decay group
            dec.insert(2, self.lstm_ln)
        params = groups(dec, hp.weight_decay, hp.decoder_lr)
        if hp.embedding_lr > 0 and not hp.weight_tying:
            params += [{"params": self.embedding.parameters(), "lr": hp.embedding_lr, "weight_decay": 0.0}]
        if hp.encoder_finetune_after > 0 and hp.encoder_lr > 0:          # F10: mirrored as written
            params += groups([self.encoder], hp.weight_decay, hp.encoder_lr)
        if hp.opt not in ("sgd", "adam", "adamw", "asgd"):
            raise ValueError("opt=%r" % (hp.opt,))
        # averaged weights (optim.py): opt="asgd" is torch.optim.ASGD, ema_decay keeps an exponential moving average beside the other three
        asgd = dict(lambd=getattr(hp, "asgd_lambd", 1e-4), alpha=getattr(hp, "asgd_alpha", 0.75), t0=getattr(hp, "asgd_t0", 1e6))
        if getattr(hp, "fused_optimizer", True):
            # one launch over every parameter tensor (csrc/optimizer.hip), gradient clipping of train.py:93-96 folded in
            from .optim import FusedOptimizer
            opt = FusedOptimizer(params, kind=hp.opt, lr=hp.decoder_lr, betas=(hp.adam_b1, hp.adam_b2), momentum=hp.momentum, nesterov=hp.nesterov,
                                 grad_clip=getattr(hp, "grad_clip", None), clip_value=getattr(hp, "clip_value", 0.0),
                                 ema_decay=getattr(hp, "ema_decay", 0.0), **asgd)
        elif hp.opt == "asgd":
            opt = torch.optim.ASGD(params, lr=hp.decoder_lr, **asgd)
        elif hp.opt == "sgd":
            opt = torch.optim.SGD(params, lr=hp.decoder_lr, momentum=hp.momentum, nesterov=hp.nesterov)
        elif hp.opt == "adam":
            opt = torch.optim.Adam(params, lr=hp.decoder_lr, betas=(hp.adam_b1, hp.adam_b2))
        else:
            opt = torch.optim.AdamW(params, lr=hp.decoder_lr, betas=(hp.adam_b1, hp.adam_b2))
        self.opt_init_lr = [pg["lr"] for pg in opt.param_groups]
        self.__dict__["_sat_optimizer"] = opt
        sched = getattr(hp, "scheduler", None)
        if sched == "step":
            self.scheduler = MultiStepLR(opt, milestones=hp.milestones, gamma=hp.lr_gamma)
        elif sched == "plateau":
            self.scheduler = ReduceLROnPlateau(opt, mode="max", factor=hp.lr_gamma, patience=hp.plateau_patience, min_lr=hp.min_lr)
        elif sched == "exp":
            self.scheduler = ExponentialLR(opt, gamma=hp.lr_gamma)
        elif sched == "cosine":
            adj = hp.epochs * hp.train_loader_len - hp.lr_warmup_steps
            t0, tm = hp.cosine_iterations, hp.cosine_multi
            if tm != 1:
                restarts = math.floor(math.log(1 - (adj * (1 - tm) / t0)) / math.log(tm))
                t0 = adj + hp.accumulate if restarts == 0 else math.ceil((adj + hp.accumulate) / ((1 - tm ** restarts) / (1 - tm)))
            else:
                restarts = math.floor(adj / t0)
                t0 = adj + hp.accumulate if restarts == 0 else math.ceil((adj + hp.accumulate) / restarts)
            self.scheduler = CosineAnnealingWarmRestarts(opt, T_0=int(t0), T_mult=int(tm), eta_min=hp.min_lr)
        elif sched == "one_cycle":
            hp.lr_warmup_steps = 0
            self.scheduler = OneCycleLR(opt, self.opt_init_lr, epochs=hp.epochs, steps_per_epoch=hp.train_loader_len,
                                        pct_start=hp.one_cycle_pct, cycle_momentum=False, div_factor=hp.one_cycle_div,
                                        final_div_factor=hp.one_cycle_fdiv)
        return opt
