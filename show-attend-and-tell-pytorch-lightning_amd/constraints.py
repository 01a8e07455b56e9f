"""Constraints on the beam search's selection step ("Constrained search"): the host half.

``resolve`` turns the public keywords ``topg`` / ``prefix`` / ``banned`` / ``no_unk`` into one checked ``SearchConstraints``
(or ``None`` when nothing constrains the search) and raises every ``ValueError`` of the specification; it touches no GPU.
The batched search (``SATDecoder._beam_search_device``) hands the result to ``sat_beam_search_constrained`` as device
arrays, the per-image loop (``SATDecoder.beam_decode``) applies the same rules with torch ops.

``resolve_history`` does the same for the rules that read what a hypothesis has already said ("History rules"):
``no_repeat_ngram`` / ``min_length`` / ``repetition_penalty`` become one checked ``HistoryRules`` (or ``None``), handed to
``sat_beam_search_history`` as a ``sat_beam_history``; ``resolve_all`` runs both.  ``resolve_groups`` checks the diverse beam search,
``resolve_required`` the words a caption must contain ("Required words"), handed to ``sat_beam_search_required``.

``SearchOptions`` names the options of a search once; ``SearchOptions.resolve`` is the one refusal sequence every caller runs before
any launch."""
import dataclasses
import inspect
import math

import torch

from . import _lib as L

SPECIALS = ("<START>", "<PAD>", "<END>", "<UNK>")


class SearchConstraints:
    """topg: 0 = off; prefix: one list of token ids per image; banned: sorted list of token ids"""

    def __init__(self, topg, prefix, banned):
        self.topg, self.prefix, self.banned = int(topg), prefix, banned
        self.max_prefix = max([len(p) for p in prefix] or [0])

    def device_struct(self, dev):
        """(sat_beam_constraints, the tensors it points into)"""
        B, keep = len(self.prefix), []
        con = L.BeamConstraints(topg=self.topg, max_prefix=self.max_prefix, n_banned=len(self.banned))
        if self.max_prefix:
            rows = [p + [0] * (self.max_prefix - len(p)) for p in self.prefix]
            pre = torch.tensor(rows, dtype=torch.int32).reshape(B, self.max_prefix).to(dev)
            plen = torch.tensor([len(p) for p in self.prefix], dtype=torch.int32).to(dev)
            con.prefix, con.prefix_len = pre.data_ptr(), plen.data_ptr()
            keep += [pre, plen]
        if self.banned:
            ban = torch.tensor(self.banned, dtype=torch.int32).to(dev)
            con.banned = ban.data_ptr()
            keep.append(ban)
        return con, keep


class HistoryRules:
    """no_repeat_ngram: 0 = off; min_length: 0 = off; repetition_penalty: 1.0 = off"""

    def __init__(self, no_repeat_ngram, min_length, repetition_penalty):
        self.no_repeat_ngram, self.min_length, self.repetition_penalty = int(no_repeat_ngram), int(min_length), float(repetition_penalty)

    def device_struct(self):
        """sat_beam_history"""
        return L.BeamHistory(no_repeat_ngram=self.no_repeat_ngram, min_length=self.min_length, repetition_penalty=self.repetition_penalty)


#: sat_beam_search_history keeps a row's history in a table of SAT_CAPTION_MAX_LEN words (include/sat_hip.h)
HISTORY_MAX_LEN = 128


def check_sample_topp(sample_method, sample_topp):
    """``sample_topp`` of "nucleus" sampling is a finite share in (0, 1] (include/sat_hip.h refuses the same values)"""
    if sample_method == "nucleus" and not (0.0 < float(sample_topp) <= 1.0):
        raise ValueError("sample_topp %r outside (0, 1] (sample_method='nucleus')" % (sample_topp,))


def check_ancestral(sample_method, beamk, graph=False, topg=None, prefix=None, banned=None, no_unk=False, no_repeat_ngram=None, min_length=None,
                    repetition_penalty=None):
    """``ValueError`` for a call that ``sample_method="ancestral"`` is not defined for (include/sat_hip.h, SAT_SAMPLE_ANCESTRAL): it draws one
    hypothesis per row (``beamk == 1``; independent samples of an image are rows of a larger batch), takes no constraint and is not
    replayed from a graph.  Touches no GPU."""
    if sample_method != "ancestral":
        return
    if int(beamk) != 1:
        raise ValueError("sample_method='ancestral' is defined for beamk=1 only (beamk=%d): repeat the images to draw several samples" % int(beamk))
    if topg is not None or prefix is not None or no_unk or (banned is not None and len(banned) > 0):
        raise ValueError("sample_method='ancestral' does not combine with topg / prefix / banned / no_unk")
    if no_repeat_ngram is not None or min_length is not None or repetition_penalty is not None:
        raise ValueError("sample_method='ancestral' does not combine with no_repeat_ngram / min_length / repetition_penalty")
    if graph:
        raise ValueError("sample_method='ancestral' is not replayed from a graph (graph=True)")


def check_mbr(rescore_method, mbr_corpus, mbr_reward, mbr_alpha, beamk, vocab_size, max_gen_length):
    """``rescore_method="MBR"`` ("Consensus reranking"): every ``ValueError`` of the consensus selection, before any
    launch; returns ``(w_cider, w_rouge, alpha)`` as floats, or ``None`` for any other method.  A corpus that was never checked is
    checked here once per state (``ReferenceCorpus.check``, one host read, remembered by its image count): a table that dropped
    n-grams would rerank by wrong document frequencies."""
    if rescore_method != "MBR":
        return None
    if mbr_corpus is None:
        raise ValueError("rescore_method='MBR' needs mbr_corpus (an evaluation.ReferenceCorpus): the document frequencies of the consensus metric")
    if int(getattr(mbr_corpus, "images", 0)) < 1:
        raise ValueError("rescore_method='MBR': mbr_corpus holds no image (ReferenceCorpus.add)")
    if int(beamk) < 1 or int(beamk) > L.MBR_MAX_HYPS:
        raise ValueError("rescore_method='MBR' is defined for beamk in 1..%d (beamk=%d)" % (L.MBR_MAX_HYPS, int(beamk)))
    if int(vocab_size) > 65535:
        raise ValueError("rescore_method='MBR': vocab_size=%d above 65535 (an n-gram key holds token + 1 in 16 bits per position)" % int(vocab_size))
    if int(max_gen_length) < 1 or int(max_gen_length) + 1 > L.CAPTION_MAX_LEN:
        raise ValueError("rescore_method='MBR' needs 1 <= max_gen_length and max_gen_length + 1 <= %d (max_gen_length=%d)"
                         % (L.CAPTION_MAX_LEN, int(max_gen_length)))
    try:
        wc, wr = (float(x) for x in mbr_reward)
        alpha = float(mbr_alpha)
    except (TypeError, ValueError):
        raise ValueError("mbr_reward=%r is (w_cider, w_rouge) and mbr_alpha=%r a number" % (mbr_reward, mbr_alpha))
    if not all(x >= 0.0 and math.isfinite(x) for x in (wc, wr, alpha)):
        raise ValueError("mbr_reward=%r and mbr_alpha=%r are finite numbers >= 0" % (mbr_reward, mbr_alpha))
    if wc == 0.0 and wr == 0.0:
        raise ValueError("mbr_reward=(0, 0): both weights are 0 (nothing to agree on)")
    if getattr(mbr_corpus, "_checked_images", None) != mbr_corpus.images:
        try:
            mbr_corpus.check()
        except L.SatHipError as e:
            raise ValueError("rescore_method='MBR': %s" % e)
    return wc, wr, alpha


def _one_prefix(p, stoi):
    if isinstance(p, str):
        ids = []
        for word in p.split():
            if word not in stoi:
                raise ValueError("prefix word %r is not in the vocabulary" % word)
            ids.append(int(stoi[word]))
        return ids
    if torch.is_tensor(p):
        p = p.reshape(-1).tolist()
    return [int(t) for t in p]


def resolve(stoi, V, B, beamk, max_gen_length, sample_method="beam", topg=None, prefix=None, banned=None, no_unk=False):
    """The checked constraints of one search over ``B`` images, or ``None`` when the search is unconstrained."""
    if topg is None and prefix is None and banned is None and not no_unk:
        return None
    ids = {s: int(stoi[s]) for s in SPECIALS}
    V, K, S = int(V), int(beamk), int(max_gen_length)
    g = 0
    if topg is not None:
        g = int(topg)
        if not 1 <= g <= V:
            raise ValueError("topg=%d outside 1..V=%d" % (g, V))
        if sample_method != "beam":
            raise ValueError("topg combines with sample_method='beam' only, not %r" % (sample_method,))
    ban = set(int(t) for t in (banned.reshape(-1).tolist() if torch.is_tensor(banned) else (banned or [])))
    if no_unk:
        ban.add(ids["<UNK>"])
    for t in sorted(ban):
        if not 0 <= t < V:
            raise ValueError("banned id %d outside [0, V=%d)" % (t, V))
    if ids["<END>"] in ban:
        raise ValueError("<END> cannot be banned: no hypothesis could finish")
    left = V - len(ban | set(ids.values()))
    if left < max(K, g or 1):
        raise ValueError("%d unmasked ids left, the search needs max(beamk, topg) = %d" % (left, max(K, g or 1)))
    if prefix is None:
        pre = [[] for _ in range(B)]
    elif isinstance(prefix, str) or torch.is_tensor(prefix) and prefix.dim() == 1 or (
            isinstance(prefix, (list, tuple)) and all(isinstance(t, int) for t in prefix)):
        pre = [_one_prefix(prefix, stoi)] * B                       # one prefix for every image
    else:
        pre = [_one_prefix(p, stoi) for p in prefix]
        if len(pre) != B:
            raise ValueError("%d prefixes for %d images" % (len(pre), B))
    names = {v: k for k, v in ids.items()}
    for b, p in enumerate(pre):
        if len(p) > S:
            raise ValueError("prefix of image %d has %d words, max_gen_length is %d" % (b, len(p), S))
        for t in p:
            if not 0 <= t < V:
                raise ValueError("prefix id %d outside [0, V=%d)" % (t, V))
            if t in names:
                raise ValueError("%s (id %d) in a prefix" % (names[t], t))
            if t in ban:
                raise ValueError("banned id %d in a prefix" % t)
    con = SearchConstraints(g, [list(p) for p in pre], sorted(ban))
    return con if (con.topg or con.max_prefix or con.banned) else None



def resolve_history(V, beamk, max_gen_length, sample_method, topg, n_banned, no_repeat_ngram=None, min_length=None, repetition_penalty=None):
    """The checked history rules of one search, or ``None`` when every rule is off (``None``, ``no_repeat_ngram=0``, ``min_length=0``,
    ``repetition_penalty=1.0``).  ``n_banned``: the banned ids that are none of the four specials.  A row loses at most one word per
    earlier position to the n-gram rule, so ``V - 4 - n_banned - max_gen_length`` selectable words must cover ``max(beamk, topg or 1)``.
    Touches no GPU."""
    n = 0 if no_repeat_ngram is None else int(no_repeat_ngram)
    m = 0 if min_length is None else int(min_length)
    theta = 1.0 if repetition_penalty is None else float(repetition_penalty)
    S = int(max_gen_length)
    if n < 0:
        raise ValueError("no_repeat_ngram=%d is negative (0 = off)" % n)
    if not 0 <= m <= S:
        raise ValueError("min_length=%d outside 0..max_gen_length=%d" % (m, S))
    if not (math.isfinite(theta) and theta > 0.0):
        raise ValueError("repetition_penalty=%r is not a positive finite number (1.0 = off)" % (repetition_penalty,))
    if n == 0 and m == 0 and theta == 1.0:
        return None
    if sample_method == "ancestral":
        raise ValueError("sample_method='ancestral' does not combine with no_repeat_ngram / min_length / repetition_penalty")
    if S + 1 > HISTORY_MAX_LEN:
        raise ValueError("the history rules need max_gen_length + 1 <= %d (max_gen_length=%d)" % (HISTORY_MAX_LEN, S))
    need = max(int(beamk), int(topg or 0) or 1)
    left = int(V) - len(SPECIALS) - int(n_banned) - S
    if left < need:
        raise ValueError("%d unmasked ids left after max_gen_length=%d blocked words, the search needs max(beamk, topg) = %d" % (left, S, need))
    return HistoryRules(n, m, theta)


class BeamGroups:
    """groups: G > 1; diversity_penalty: lambda >= 0 ("Diverse beam search")"""

    def __init__(self, groups, diversity_penalty):
        self.groups, self.diversity_penalty = int(groups), float(diversity_penalty)

    def device_struct(self):
        """sat_beam_groups"""
        return L.BeamGroups(groups=self.groups, diversity_penalty=self.diversity_penalty)


#: beam_group_select_kernel keeps the words kept at a step in a table of this many entries
GROUPS_MAX_BEAMK = 1024


def resolve_groups(beamk, beam_groups=None, diversity_penalty=0.5, sample_method="beam", decoder_noise=None, topg=None, prefix=None, graph=False,
                   batched=True, V=None):
    """The checked groups of one search, or ``None`` when the beam is not split (``beam_groups`` ``None``, 0 or 1: today's search,
    whatever ``diversity_penalty`` says).  Every ``ValueError`` of the diverse beam search ("Diverse beam search"), each
    naming its argument; ``batched=False`` is the per-image loop ``beam_decode``, which has no groups.  Touches no GPU."""
    if beam_groups is None:
        return None
    G, K = int(beam_groups), int(beamk)
    if G < 0:
        raise ValueError("beam_groups=%d is negative (None, 0 or 1 = off)" % G)
    if G <= 1:
        return None
    try:
        lam = float(diversity_penalty)
    except (TypeError, ValueError):
        raise ValueError("diversity_penalty=%r is not a number" % (diversity_penalty,))
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("diversity_penalty=%r is not a finite number >= 0" % (diversity_penalty,))
    if not batched:
        raise ValueError("beam_groups=%d runs in the batched search only (beam_decode_batched), not in the per-image loop beam_decode" % G)
    if sample_method != "beam":
        raise ValueError("beam_groups combines with sample_method='beam' only, not %r" % (sample_method,))
    if decoder_noise:
        raise ValueError("beam_groups does not combine with decoder_noise=%r" % (decoder_noise,))
    if topg is not None:
        raise ValueError("beam_groups does not combine with topg=%r" % (topg,))
    if prefix is not None:
        raise ValueError("beam_groups does not combine with a forced prefix (prefix=%r)" % (prefix,))
    if graph:
        raise ValueError("beam_groups is not replayed from a graph (graph=True)")
    if K < 1 or K % G != 0:
        raise ValueError("beam_groups=%d does not divide beamk=%d" % (G, K))
    if K > GROUPS_MAX_BEAMK:
        raise ValueError("beam_groups needs beamk <= %d (beamk=%d)" % (GROUPS_MAX_BEAMK, K))
    if V is not None and K // G > int(V):
        raise ValueError("beam_groups=%d: beamk / beam_groups = %d above V=%d" % (G, K // G, int(V)))
    return BeamGroups(G, lam)


class Required:
    """words: one list of distinct token ids per image ("Required words"); an empty list searches that image as today"""

    def __init__(self, words):
        self.words = [list(w) for w in words]
        self.max_required = max([len(w) for w in self.words] or [0])

    def device_struct(self, dev):
        """(sat_beam_required, the tensors it points into)"""
        C = self.max_required
        rows = [w + [0] * (C - len(w)) for w in self.words]
        words = torch.tensor(rows, dtype=torch.int32).reshape(len(rows), C).to(dev)
        n_words = torch.tensor([len(w) for w in self.words], dtype=torch.int32).to(dev)
        return L.BeamRequired(max_required=C, words=words.data_ptr(), n_words=n_words.data_ptr()), [words, n_words]


#: sat_beam_search_required: SAT_BEAM_REQUIRED_MAX words per image, beamk <= SAT_BEAM_REQUIRED_MAX_K (include/sat_hip.h)
REQUIRED_MAX = 8
REQUIRED_MAX_BEAMK = 256


def _one_required(r, stoi):
    if torch.is_tensor(r):
        r = r.reshape(-1).tolist()
    ids = []
    for word in (r.split() if isinstance(r, str) else r):
        if isinstance(word, str) and stoi is not None:
            if word not in stoi:
                raise ValueError("required word %r is not in the vocabulary" % word)
            word = int(stoi[word])
        ids.append(word if isinstance(word, str) else int(word))
    return ids


def _required_lists(required, B, stoi):
    """one list per image from one list / string for every image, or one list / string per image"""
    if isinstance(required, str) or torch.is_tensor(required) and required.dim() == 1 or (
            isinstance(required, (list, tuple)) and all(isinstance(t, int) for t in required)):
        return [_one_required(required, stoi)] * B
    req = [_one_required(r, stoi) for r in required]
    if len(req) != B:
        raise ValueError("required: %d word lists for %d images" % (len(req), B))
    return req


def resolve_required(stoi, V, B, beamk, max_gen_length, required=None, sample_method="beam", decoder_noise=None, topg=None, prefix=None, banned=None,
                     no_unk=False, beam_groups=None, graph=False, batched=True):
    """The checked required words of one search over ``B`` images ("Required words"), or ``None`` when nothing is required
    (``None``, ``[]``, or an empty list / string for every image: today's search).  ``required``: one list of ids or one string of words
    for every image, or one list / string per image (ragged); a string is split on whitespace, as ``prefix`` is.  Every ``ValueError`` of
    the feature, each naming its argument; ``batched=False`` is the per-image loop ``beam_decode``.  Touches no GPU."""
    if required is None:
        return None
    V, K, S, B = int(V), int(beamk), int(max_gen_length), int(B)
    req = _required_lists(required, B, stoi)
    if not any(req):
        return None
    if not batched:
        raise ValueError("required words run in the batched search only (beam_decode_batched, max_gen_length >= 1), not in the per-image loop beam_decode")
    ids = {s: int(stoi[s]) for s in SPECIALS}
    names = {v: k for k, v in ids.items()}
    ban = set(int(t) for t in (banned.reshape(-1).tolist() if torch.is_tensor(banned) else (banned or [])))
    if no_unk:
        ban.add(ids["<UNK>"])
    for b, words in enumerate(req):
        for t in words:
            if not 0 <= t < V:
                raise ValueError("required id %d outside [0, V=%d)" % (t, V))
            if t in names:
                raise ValueError("%s (id %d) among the required words" % (names[t], t))
            if t in ban:
                raise ValueError("banned id %d among the required words" % t)
        if len(set(words)) != len(words):
            raise ValueError("required words of image %d repeat an id (%r)" % (b, words))
        if len(words) > REQUIRED_MAX:
            raise ValueError("required: image %d has %d words, at most %d" % (b, len(words), REQUIRED_MAX))
        if len(words) > S:
            raise ValueError("required: image %d has %d words, max_gen_length is %d" % (b, len(words), S))
    if K > REQUIRED_MAX_BEAMK:
        raise ValueError("required needs beamk <= %d (beamk=%d)" % (REQUIRED_MAX_BEAMK, K))
    if sample_method != "beam":
        raise ValueError("required combines with sample_method='beam' only, not %r" % (sample_method,))
    if decoder_noise:
        raise ValueError("required does not combine with decoder_noise=%r" % (decoder_noise,))
    if topg is not None:
        raise ValueError("required does not combine with topg=%r" % (topg,))
    if prefix is not None:
        raise ValueError("required does not combine with a forced prefix (prefix=%r)" % (prefix,))
    if beam_groups is not None and int(beam_groups) > 1:
        raise ValueError("required does not combine with beam_groups=%d" % int(beam_groups))
    if graph:
        raise ValueError("required is not replayed from a graph (graph=True)")
    if S + 1 > HISTORY_MAX_LEN:
        raise ValueError("required needs max_gen_length + 1 <= %d (max_gen_length=%d): the history tables" % (HISTORY_MAX_LEN, S))
    left = V - len(SPECIALS) - len(ban - set(ids.values())) - S
    if left < K:
        raise ValueError("required: %d unmasked ids left after max_gen_length=%d blocked words, the search needs beamk = %d" % (left, S, K))
    return Required(req)


def required_coverage(captions, required, stoi=None):
    """Per image, the fraction of its required words that its caption says (1.0 for an image without required words).  ``captions``: one
    caption per image, a list of words or ids or a string; ``required``: what ``resolve_required`` takes.  With ``stoi`` the words of both
    are compared as ids (a word outside the vocabulary is <UNK>), otherwise as given.  A host helper: no GPU, no checks of the search."""
    def norm(seq):
        seq = seq.split() if isinstance(seq, str) else (seq.reshape(-1).tolist() if torch.is_tensor(seq) else list(seq))
        if stoi is None:
            return seq
        return [int(stoi.get(t, stoi["<UNK>"])) if isinstance(t, str) else int(t) for t in seq]
    B = len(captions)
    req = [[] for _ in range(B)] if required is None else _required_lists(required, B, None)
    out = []
    for cap, words in zip(captions, req):
        said, words = set(norm(cap)), norm(words)
        out.append(sum(1 for w in words if w in said) / len(words) if words else 1.0)
    return out


def resolve_all(stoi, V, B, beamk, max_gen_length, sample_method="beam", topg=None, prefix=None, banned=None, no_unk=False, no_repeat_ngram=None,
                min_length=None, repetition_penalty=None):
    """``(resolve(...), resolve_history(...))``: every ``ValueError`` of both, before any launch"""
    con = resolve(stoi, V, B, beamk, max_gen_length, sample_method, topg, prefix, banned, no_unk)
    special = {int(stoi[s]) for s in SPECIALS}
    n_banned = len([t for t in con.banned if t not in special]) if con is not None else 0
    return con, resolve_history(V, beamk, max_gen_length, sample_method, topg, n_banned, no_repeat_ngram, min_length, repetition_penalty)


@dataclasses.dataclass(frozen=True, eq=False)
class SearchOptions:
    """The options of one search (``SATDecoder.beam_decode_batched`` documents them), with the defaults of every public signature.
    Callers build one from their own keywords (``from_kwargs(locals())``) and pass it on whole, so no option travels by position."""
    sample_method: str = "beam"
    sample_topk: int = 3
    sample_topp: float = 0.9
    decoder_noise: object = None
    seed: object = None
    gumbel: object = None
    normals: object = None
    graph: bool = False
    topg: object = None
    prefix: object = None
    banned: object = None
    no_unk: bool = False
    no_repeat_ngram: object = None
    min_length: object = None
    repetition_penalty: object = None
    beam_groups: object = None
    diversity_penalty: float = 0.5
    required: object = None

    @classmethod
    def from_kwargs(cls, kw, **over):
        """the options among the keywords ``kw`` (a caller's ``locals()``), ``over`` on top; ``sample_method`` as a string"""
        names = {f.name for f in dataclasses.fields(cls)}
        o = {k: v for k, v in dict(kw, **over).items() if k in names}
        if "sample_method" in o:
            o["sample_method"] = str(o["sample_method"])
        return cls(**o)

    def kwargs(self, fn):
        """the options the public function ``fn`` takes one by one, as keywords"""
        names = inspect.signature(fn).parameters
        return {f.name: getattr(self, f.name) for f in dataclasses.fields(self) if f.name in names}

    def resolve(self, stoi, V, B, beamk, max_gen_length, batched=True):
        """Every ``ValueError`` of a search over ``B`` images, before any launch and touching no GPU, in one order: ``sample_topp``, what
        "ancestral" sampling refuses, the constraints and history rules, the groups, the required words.  ``batched=False`` is the
        per-image loop ``beam_decode``, which has neither groups nor required words.  Returns ``(con, hist, grp, req)``, each ``None``
        when off."""
        assert self.sample_method in L.SAMPLE_METHODS
        check_sample_topp(self.sample_method, self.sample_topp)
        check_ancestral(self.sample_method, beamk, self.graph, self.topg, self.prefix, self.banned, self.no_unk, self.no_repeat_ngram, self.min_length,
                        self.repetition_penalty)
        con, hist = resolve_all(stoi, V, B, beamk, max_gen_length, self.sample_method, self.topg, self.prefix, self.banned, self.no_unk, self.no_repeat_ngram,
                                self.min_length, self.repetition_penalty)
        grp = resolve_groups(beamk, self.beam_groups, self.diversity_penalty, self.sample_method, self.decoder_noise, self.topg, self.prefix, self.graph,
                             batched=batched, V=V)
        req = resolve_required(stoi, V, B, beamk, max_gen_length, self.required, self.sample_method, self.decoder_noise, self.topg, self.prefix, self.banned,
                               self.no_unk, self.beam_groups, self.graph, batched=batched)
        return con, hist, grp, req
