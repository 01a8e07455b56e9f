"""The reference's ``evaluate.ipynb`` without the host tail: a validation batch stays on the device from image to metric statistics.

``SAT.val_batch`` reads the search's back-trace (attention history included) to the host, rebuilds Python lists, counts n-grams four
times over and loops over B x R tiny torch ops for the cosine.  Here the winning hypothesis of every image is picked and traced back
by ``sat_beam_select``, ``sat_caption_stats`` produces the integers that corpus BLEU / GLEU sum per segment, ``sat_caption_cosine`` the
best mean-embedding cosine (csrc/caption_score.hip); what reaches the host is one vector of 14 numbers per batch -- or per split:

* ``caption_tokens``    encoder + batched search + selection: device tensors, no copy to the host, no synchronisation, capturable;
* ``val_batch_stats``   the device counterpart of ``SAT.val_batch``: a ``CaptionStats`` (sums over the images of the batch);
* ``evaluate``          a loader's batches: the notebook's mean of per-batch metrics AND the corpus-level score of the whole split
                        (dev/todo.txt: "add the val_epoch_end, sum the nom/dem"), read from the device once at the end;
* ``random_search``     the notebook's random search over decode parameters, same draws in the same order.

Opt-in, ``corpus=ReferenceCorpus``: CIDEr-D and ROUGE-L (csrc/caption_consensus.hip; ``metrics.cider_d`` / ``metrics.rouge_l`` are the
specification).  The document frequency of every 1..4-gram of a split's references is built once into a hash table on the device
(``ReferenceCorpus``) and stays there; ``consensus_scores`` scores a batch against it in the same enqueue as the statistics above, and
``val_batch_stats`` / ``evaluate`` / ``random_search`` carry the two sums along.  Without ``corpus`` nothing changes.

Opt-in, ``chrf=VocabChars``: chrF (csrc/caption_chrf.hip; ``metrics.chrf`` is the specification), the one metric here that looks inside
words.  The vocabulary's spelling is put on the device once (``VocabChars``); ``chrf_scores`` scores a batch over the characters of its
tokens in one launch, and the same three carry the sum along.  Without ``chrf`` nothing changes.

Opt-in, ``rescore_method="MBR"`` with ``mbr_corpus=ReferenceCorpus``: consensus reranking of the finished beam (csrc/caption_mbr.hip;
``metrics.consensus_utilities`` is the specification).  ``finished_hypotheses`` traces every finished hypothesis back on the device,
``consensus_utilities`` scores them against each other, ``select_hypotheses`` gathers the winner: three launches, no host read.  The
reference's four rules (None / "LN" / "WR" / "BAR") stay on ``sat_beam_select``.

Opt-in, ``with_diversity=True``: how different the finished hypotheses of an image are (csrc/caption_diversity.hip;
``metrics.diversity_stats`` is the specification): distinct-n, mBLEU and the share of unique captions over ``finished_hypotheses`` of the
same search buffers, and the vocabulary the selected captions use.  ``diversity_statistics`` is one launch, ``val_batch_stats`` hangs a
``DiversityStats`` on its ``CaptionStats``, ``evaluate`` sums them over the split and reads them once.  Without the flag nothing changes.
"""
import numpy as np
import torch

from . import _lib as L
from . import constraints
from . import metrics

#: the reference's BLEU weights (model.py:651-654), bleu3 as written there
BLEU_WEIGHTS = {"bleu1": (1, 0, 0, 0), "bleu2": (0.5, 0.5, 0, 0), "bleu3": (0.33, 0.33, 0.33, 0), "bleu4": (0.25, 0.25, 0.25, 0.25)}
METRIC_KEYS = ("bleu1", "bleu2", "bleu3", "bleu4", "cosine_similarity", "gleu", "perplexity")
#: evaluate.ipynb's result table and parameter ranges
HEADERS = ["beamk", "temperature", "sample_method", "decoder_noise", "rescore_method", "rescore_reward"] + list(METRIC_KEYS)
NOTEBOOK_SPACE = dict(beamks=[5, 20], temperatures=(0.7, 1.2), sample_methods=["beam", "multinomial"], decoder_noises=[0.0],
                      rescore_methods=["LN", "BAR"], rescore_rewards=(0.6, 1.3), max_gen_length=32)


def finished_hypotheses(buffers, pad_id):
    """``sat_beam_hypotheses`` on the buffers ``SATDecoder._beam_search_device`` returns: the back-trace of EVERY finished hypothesis
    on the device, ``(hyp_tokens (B, beamk, S + 1) int32 padded with pad_id, hyp_len (B, beamk) int32)`` in append order; the slots
    beyond ``fin_count`` are empty.  One launch, no host read."""
    tok_in = buffers["tok_in"]
    L.require_gpu(tok_in)
    S, (B, K) = tok_in.shape[0] - 2, tok_in.shape[1:]
    hyp_tokens = torch.empty(B, K, S + 1, dtype=torch.int32, device=tok_in.device)
    hyp_len = torch.empty(B, K, dtype=torch.int32, device=tok_in.device)
    L.check(L.lib().sat_beam_hypotheses(L.ptr(tok_in), L.ptr(buffers["prev_row"]), L.ptr(buffers["fin_count"]), L.ptr(buffers["fin_step"]),
                                        L.ptr(buffers["fin_row"]), B, K, S, int(pad_id), L.ptr(hyp_tokens), L.ptr(hyp_len), L.stream_ptr()),
            "sat_beam_hypotheses")
    return hyp_tokens, hyp_len


def consensus_utilities(hyp_tokens, hyp_len, counts, logp, corpus, reward=(1.0, 0.0), alpha=0.0, sigma=6.0):
    """``sat_caption_mbr``: ``(utilities (B, K) float64, winner (B) int32)`` on the device of the hypotheses ``hyp_tokens (B, K, W)`` /
    ``hyp_len (B, K)`` / ``counts (B)`` (int32) with raw scores ``logp (B, K)`` float32 (``None`` goes with ``alpha=0``), against the
    document frequencies of ``corpus``; ``metrics.consensus_utilities`` is the specification.  One launch, no host read."""
    L.require_gpu(hyp_tokens, hyp_len, counts)
    for t in (hyp_tokens, hyp_len, counts):
        assert t.dtype == torch.int32 and t.is_contiguous()
    if logp is not None:
        L.require_gpu(logp)
        assert logp.dtype == torch.float32 and logp.is_contiguous()
    if corpus.images < 1 or corpus._table is None:
        raise ValueError("consensus_utilities: the corpus holds no image (ReferenceCorpus.add)")
    B, K, W = hyp_tokens.shape
    utilities = torch.empty(B, K, dtype=torch.float64, device=hyp_tokens.device)
    winner = torch.empty(B, dtype=torch.int32, device=hyp_tokens.device)
    L.check(L.lib().sat_caption_mbr(L.ptr(hyp_tokens), L.ptr(hyp_len), L.ptr(counts), L.ptr(logp), B, K, W, L.ptr(corpus._table), corpus.capacity,
                                    corpus.images, float(sigma), float(reward[0]), float(reward[1]), float(alpha), L.ptr(utilities), L.ptr(winner),
                                    L.stream_ptr()), "sat_caption_mbr")
    return utilities, winner


def diversity_statistics(hyp_tokens, hyp_len, counts, per_hypothesis=False):
    """``sat_caption_diversity``: ``stats (B, 20) int32`` on the device of the hypotheses ``hyp_tokens (B, K, W)`` / ``hyp_len (B, K)`` /
    ``counts (B)`` (int32, the layout ``finished_hypotheses`` leaves) -- the columns of ``metrics.diversity_stats``, which is the
    specification; ``per_hypothesis``: also ``per_hyp (B, K, 10) int32``, ``metrics.diversity_per_hypothesis``.  One launch, no host read."""
    L.require_gpu(hyp_tokens, hyp_len, counts)
    for t in (hyp_tokens, hyp_len, counts):
        assert t.dtype == torch.int32 and t.is_contiguous()
    B, K, W = hyp_tokens.shape
    assert tuple(hyp_len.shape) == (B, K) and tuple(counts.shape) == (B,), "hyp_len is (B, K), counts is (B)"
    stats = torch.empty(B, L.DIVERSITY_STATS, dtype=torch.int32, device=hyp_tokens.device)
    per_hyp = torch.empty(B, K, 10, dtype=torch.int32, device=hyp_tokens.device) if per_hypothesis else None
    L.check(L.lib().sat_caption_diversity(L.ptr(hyp_tokens), L.ptr(hyp_len), L.ptr(counts), B, K, W, L.ptr(stats), L.ptr(per_hyp), L.stream_ptr()),
            "sat_caption_diversity")
    return (stats, per_hyp) if per_hypothesis else stats


def vocabulary_usage(tokens, lengths, vocab_size, counts=None):
    """``sat_caption_vocab_usage``: ``counts (vocab_size) int32`` on the device, how often each word occurs in the captions ``tokens
    (B, W)`` / ``lengths (B)`` (int32); ids outside the vocabulary are skipped.  A given ``counts`` is added to.  One launch (and the
    clear of a fresh ``counts``), no host read."""
    L.require_gpu(tokens, lengths)
    for t in (tokens, lengths):
        assert t.dtype == torch.int32 and t.is_contiguous()
    B, W = tokens.shape
    if counts is None:
        counts = torch.zeros(int(vocab_size), dtype=torch.int32, device=tokens.device)
    L.require_gpu(counts)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == int(vocab_size)
    L.check(L.lib().sat_caption_vocab_usage(L.ptr(tokens), L.ptr(lengths), W, B, int(vocab_size), L.ptr(counts), L.stream_ptr()), "sat_caption_vocab_usage")
    return counts


class DiversityStats:
    """Sums over images of the columns of ``sat_caption_diversity``: ``sums`` (20,) int64 and ``vocab_counts`` (vocab_size,) int64 (how
    often the selected captions use each word) on the device, ``images`` and ``vocab_size`` host ints.  ``a + b`` adds; ``metrics()``
    reads the device once and returns ``metrics.diversity_from_stats`` with ``vocabulary`` = the number of words used at least once."""

    def __init__(self, sums, vocab_counts, images, vocab_size):
        self.sums, self.vocab_counts, self.images, self.vocab_size = sums, vocab_counts, int(images), int(vocab_size)

    def __add__(self, other):
        if self.vocab_size != other.vocab_size:
            raise ValueError("DiversityStats: vocabularies of %d and %d words" % (self.vocab_size, other.vocab_size))
        return DiversityStats(self.sums + other.sums, self.vocab_counts + other.vocab_counts, self.images + other.images, self.vocab_size)

    def vector(self):
        """(21,) int64 on the device: the 20 sums, then the number of words with a non-zero count"""
        return torch.cat([self.sums, (self.vocab_counts != 0).sum(dtype=torch.int64).reshape(1)])

    def metrics(self):
        v = self.vector().cpu().tolist()                                      # the one host read
        return metrics.diversity_from_stats(v[:L.DIVERSITY_STATS], vocab_used=v[L.DIVERSITY_STATS])


def select_hypotheses(buffers, pad_id, rescore_method=None, rescore_reward=0.5, with_alpha=False, mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0):
    """``sat_beam_select`` on the buffers ``SATDecoder._beam_search_device`` returns: the best hypothesis of every image as
    ``dict(tokens (B, S + 1) int32 padded with pad_id, lengths (B) int32, scores (B) rescored, raw (B), steps (B), alphas (B, S, L) or None)``.
    ``rescore_method="MBR"``: consensus reranking against ``mbr_corpus`` (``sat_beam_hypotheses`` -> ``sat_caption_mbr`` ->
    ``sat_beam_select_at``, three launches and no host read); ``scores`` is then the winner's utility."""
    tok_in, alpha_hist = buffers["tok_in"], buffers["alpha_hist"]
    S, (B, K), Lc = tok_in.shape[0] - 2, tok_in.shape[1:], alpha_hist.shape[-1]
    mbr = constraints.check_mbr(rescore_method, mbr_corpus, mbr_reward, mbr_alpha, K, 1, S)      # the caller's vocabulary built the corpus
    if mbr is None and rescore_method not in L.RESCORE:
        raise ValueError("rescore_method=%r (None, 'LN', 'WR', 'BAR', 'MBR')" % (rescore_method,))
    L.require_gpu(tok_in)
    dev = tok_in.device
    i32 = dict(dtype=torch.int32, device=dev); f32 = dict(dtype=torch.float32, device=dev)
    out = dict(tokens=torch.empty(B, S + 1, **i32), lengths=torch.empty(B, **i32), scores=torch.empty(B, **f32), raw=torch.empty(B, **f32),
               steps=torch.empty(B, **i32), alphas=torch.empty(B, S, Lc, **f32) if with_alpha else None)
    if mbr is not None:
        hyp_tokens, hyp_len = finished_hypotheses(buffers, pad_id)
        utilities, winner = consensus_utilities(hyp_tokens, hyp_len, buffers["fin_count"], buffers["fin_score"], mbr_corpus, mbr[:2], mbr[2])
        L.check(L.lib().sat_beam_select_at(L.ptr(tok_in), L.ptr(buffers["prev_row"]), L.ptr(buffers["fin_count"]), L.ptr(buffers["fin_step"]),
                                           L.ptr(buffers["fin_row"]), L.ptr(buffers["fin_score"]), L.ptr(alpha_hist) if with_alpha else None,
                                           L.ptr(winner), L.ptr(utilities), B, K, S, Lc, int(pad_id), L.ptr(out["tokens"]), L.ptr(out["lengths"]),
                                           L.ptr(out["scores"]), L.ptr(out["raw"]), L.ptr(out["steps"]), L.ptr(out["alphas"]), L.stream_ptr()),
                "sat_beam_select_at")
        out.update(hyp_tokens=hyp_tokens, hyp_len=hyp_len, utilities=utilities, winner=winner)
        return out
    L.check(L.lib().sat_beam_select(L.ptr(tok_in), L.ptr(buffers["prev_row"]), L.ptr(buffers["fin_count"]), L.ptr(buffers["fin_step"]),
                                    L.ptr(buffers["fin_row"]), L.ptr(buffers["fin_score"]), L.ptr(buffers["fin_mean"]),
                                    L.ptr(alpha_hist) if with_alpha else None, B, K, S, Lc, L.RESCORE[rescore_method], float(rescore_reward), int(pad_id),
                                    L.ptr(out["tokens"]), L.ptr(out["lengths"]), L.ptr(out["scores"]), L.ptr(out["raw"]), L.ptr(out["steps"]),
                                    L.ptr(out["alphas"]), L.stream_ptr()), "sat_beam_select")
    return out


@torch.no_grad()
def caption_tokens(model, img, beamk=3, max_gen_length=32, temperature=1.0, sample_method="beam", sample_topk=3, decoder_noise=None,
                   rescore_method=None, rescore_reward=0.5, seed=None, graph=False, topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None,
                   mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0, corpus=None, beam_groups=None, diversity_penalty=0.5, required=None):
    """``SAT.caption(..., return_all=False)`` with the result left on the device: ``(tokens (B, max_gen_length + 1) int32 padded with
    <PAD>, lengths (B) int32, scores (B), perplexities (B))``.  Nothing is copied to the host and nothing synchronises.
    ``topg`` / ``prefix`` / ``banned`` / ``no_unk`` constrain the search (``SATDecoder.beam_decode_batched``); ``sample_topp`` belongs to
    ``sample_method="nucleus"``; ``sample_method="ancestral"`` (``beamk=1``, no constraint, no graph) is pure sampling;
    ``no_repeat_ngram`` / ``min_length`` / ``repetition_penalty`` are the history rules ("History rules").
    ``rescore_method="MBR"`` with ``mbr_corpus`` (``corpus`` when that is None) / ``mbr_reward`` / ``mbr_alpha``: consensus reranking
    ("Consensus reranking"); ``scores`` is then the utility.  ``beam_groups`` / ``diversity_penalty``: the diverse beam
    search ("Diverse beam search"); ``required``: the words every caption must contain ("Required words").
    Launches only, like the rest."""
    opt = constraints.SearchOptions.from_kwargs(locals())
    _, sel, ppl = _search_and_select(model, img, opt, beamk, max_gen_length, temperature, rescore_method, rescore_reward, mbr_corpus, mbr_reward, mbr_alpha,
                                     corpus)
    return sel["tokens"], sel["lengths"], sel["scores"], ppl


def _search_and_select(model, img, opt, beamk, max_gen_length, temperature, rescore_method, rescore_reward, mbr_corpus, mbr_reward, mbr_alpha, corpus):
    """``caption_tokens`` with the search buffers kept: ``(buffers, select_hypotheses' dict, perplexities (B))``"""
    if int(max_gen_length) < 1:
        raise ValueError("caption_tokens: max_gen_length >= 1 (the batched search)")
    mbr_corpus = corpus if mbr_corpus is None else mbr_corpus
    constraints.check_mbr(rescore_method, mbr_corpus, mbr_reward, mbr_alpha, beamk, model.hp.vocab_size, max_gen_length)      # refuse before any launch
    opt.resolve(model.hp.vocab_stoi, model.hp.vocab_size, img.shape[0], beamk, max_gen_length)                                   # refuse before any launch
    model.eval()
    ann_bld, _ = model.encode(img)
    o = model._beam_search_device(ann_bld.contiguous(), beamk, max_gen_length, temperature, options=opt)
    sel = select_hypotheses(o, model.pad_idx, rescore_method, rescore_reward, mbr_corpus=mbr_corpus, mbr_reward=mbr_reward, mbr_alpha=mbr_alpha)
    ppl = torch.exp(-sel["raw"] / sel["steps"].float())                      # model.py:415
    return o, sel, ppl


def caption_statistics(tokens, lengths, refs, ref_lengths, embedding):
    """``(stats (B, 12) int32, best_cosine (B) float32)`` of hypotheses ``tokens (B, W)`` / ``lengths (B)`` against references
    ``refs (B, R, T)`` / ``ref_lengths (B, R)`` (all int32, on the device; layouts: include/sat_hip.h, sat_caption_stats)."""
    L.require_gpu(tokens, lengths, refs, ref_lengths, embedding)
    for t in (tokens, lengths, refs, ref_lengths):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert embedding.dtype == torch.float32 and embedding.is_contiguous()
    B, W = tokens.shape
    _, R, T = refs.shape
    V, m = embedding.shape
    stats = torch.empty(B, 12, dtype=torch.int32, device=tokens.device)
    best = torch.empty(B, dtype=torch.float32, device=tokens.device)
    lib = L.lib()
    L.check(lib.sat_caption_stats(L.ptr(tokens), L.ptr(lengths), W, L.ptr(refs), L.ptr(ref_lengths), B, R, T, L.ptr(stats), L.stream_ptr()),
            "sat_caption_stats")
    L.check(lib.sat_caption_cosine(L.ptr(tokens), L.ptr(lengths), W, L.ptr(refs), L.ptr(ref_lengths), B, R, T, L.ptr(embedding), V, m, L.ptr(best),
                                   L.stream_ptr()), "sat_caption_cosine")
    return stats, best


CONSENSUS_KEYS = ("cider", "rouge_l")
MAX_VOCAB = 65535          # an n-gram key holds (token + 1) in 16 bits per position (include/sat_hip.h)


def _pow2_at_least(x):
    return 1 << max(0, int(x) - 1).bit_length()


class ReferenceCorpus:
    """The n-gram document-frequency table of a split's references on the device (include/sat_hip.h, sat_ngram_table_add).

    ``capacity``: slots of the hash table, a power of two, honoured as given; by default the smallest power of two >= 2 x the n-gram
    positions announced by ``expected_positions`` (the constructor's, or ``from_dataset``'s count; 2^16 positions when none is
    announced).  The table is allocated at the first ``add`` (or ``clear``); every ``add`` is one launch.  ``images`` is a host int;
    ``check()`` is the one host read."""

    DEFAULT_POSITIONS = 1 << 16

    def __init__(self, vocab_size, capacity=None, device="cuda", expected_positions=None):
        if int(vocab_size) < 1 or int(vocab_size) > MAX_VOCAB:
            raise ValueError("ReferenceCorpus: vocab_size=%d (1..%d: an n-gram key holds token + 1 in 16 bits per position)" % (vocab_size, MAX_VOCAB))
        if capacity is not None and (int(capacity) < 1 or int(capacity) & (int(capacity) - 1)):
            raise ValueError("ReferenceCorpus: capacity=%d is not a power of two" % capacity)
        self.vocab_size, self.device, self.images = int(vocab_size), torch.device(device), 0
        self.capacity = int(capacity) if capacity is not None else _pow2_at_least(2 * int(expected_positions or self.DEFAULT_POSITIONS))
        self._table = self._flag = None
        self._checked_images = None            # the image count at the last check() that passed

    def _allocate(self):
        if self.device.type != "cuda":
            raise L.SatHipError("sat_amd computes on the GPU only: ReferenceCorpus on %s (no CPU fallback)" % self.device)
        nbytes = L.lib().sat_ngram_table_bytes(self.capacity)
        if nbytes == 0:
            L.check(1, "sat_ngram_table_bytes")
        self._table = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._flag = torch.empty(1, dtype=torch.int32, device=self.device)

    def clear(self):
        """empties the table and the error flag (launches only; the first call allocates): the corpus holds no image again"""
        if self._table is None:
            self._allocate()
        L.check(L.lib().sat_ngram_table_clear(L.ptr(self._table), self.capacity, L.stream_ptr()), "sat_ngram_table_clear")
        self._flag.zero_()
        self.images = 0
        return self

    def add(self, refs, ref_lengths):
        """the references ``refs (B, R, T)`` / ``ref_lengths (B, R)`` (any integer dtype, device or host) of B more images: one launch"""
        if self._table is None:
            self.clear()
        refs = torch.as_tensor(refs).to(device=self.device, dtype=torch.int32).contiguous()
        ref_lengths = torch.as_tensor(ref_lengths).to(device=self.device, dtype=torch.int32).contiguous()
        B, R, T = refs.shape
        assert tuple(ref_lengths.shape) == (B, R), "ref_lengths is (B, R)"
        L.check(L.lib().sat_ngram_table_add(L.ptr(refs), L.ptr(ref_lengths), B, R, T, L.ptr(self._table), self.capacity, L.ptr(self._flag),
                                            L.stream_ptr()), "sat_ngram_table_add")
        self.images += B
        return self

    @staticmethod
    def positions(lengths):
        """the number of (n, position) pairs, n = 1..4, of references ``c[1:l]`` with the given stored lengths ``l``"""
        l = torch.as_tensor(lengths).to(torch.int64).reshape(-1).clamp(min=1) - 1
        return int(sum((l - n).clamp(min=0).sum() for n in range(4)))

    @classmethod
    def from_dataset(cls, ds, vocab_size=None, capacity=None, device="cuda", chunk=1024):
        """the corpus of ``ds.encoded_captions (N, R, T)`` / ``ds.lengths (N, R)``, fed in chunks of ``chunk`` images; no image is touched"""
        caps, lens = torch.as_tensor(ds.encoded_captions), torch.as_tensor(ds.lengths)
        if vocab_size is None:
            vocab_size = len(ds.vocab_stoi) if hasattr(ds, "vocab_stoi") else int(caps.max()) + 1
        rc = cls(vocab_size, capacity, device, expected_positions=cls.positions(lens))
        for i in range(0, caps.shape[0], int(chunk)):
            rc.add(caps[i:i + chunk], lens[i:i + chunk])
        return rc

    def check(self):
        """reads the error flag (the one host read): raises if an ``add`` found the table full and dropped n-grams"""
        if self._flag is not None and int(self._flag.item()) != 0:
            raise L.SatHipError("ReferenceCorpus: the table overflowed (capacity %d): document frequencies are incomplete; "
                                "rebuild with a larger capacity" % self.capacity)
        self._checked_images = self.images
        return self

    def to_dict(self):
        """``{n-gram tuple: document frequency}`` on the host (tests, debugging)"""
        if self._table is None:
            return {}
        host = self._table.cpu().numpy()
        keys = host[:8 * self.capacity].view(np.uint64)
        counts = host[8 * self.capacity:].view(np.uint32)
        out = {}
        for k, c in zip(keys[keys != 0].tolist(), counts[keys != 0].tolist()):
            gram = []
            while k:
                gram.append((k & 0xFFFF) - 1); k >>= 16
            out[tuple(gram)] = c
        return out


def consensus_scores(tokens, lengths, refs, ref_lengths, corpus, sigma=6.0):
    """``(B, 2)`` float64 on the device, ``[CIDEr-D, ROUGE-L]`` per image, of hypotheses ``tokens (B, W)`` / ``lengths (B)`` against
    ``refs (B, R, T)`` / ``ref_lengths (B, R)`` (int32, on the device) with the document frequencies of ``corpus``."""
    L.require_gpu(tokens, lengths, refs, ref_lengths)
    for t in (tokens, lengths, refs, ref_lengths):
        assert t.dtype == torch.int32 and t.is_contiguous()
    if corpus.images < 1 or corpus._table is None:
        raise ValueError("consensus_scores: the corpus holds no image (ReferenceCorpus.add)")
    B, W = tokens.shape
    _, R, T = refs.shape
    scores = torch.empty(B, 2, dtype=torch.float64, device=tokens.device)
    L.check(L.lib().sat_caption_consensus(L.ptr(tokens), L.ptr(lengths), W, L.ptr(refs), L.ptr(ref_lengths), B, R, T, L.ptr(corpus._table),
                                          corpus.capacity, corpus.images, float(sigma), L.ptr(scores), L.stream_ptr()), "sat_caption_consensus")
    return scores


CHRF_KEYS = ("chrf",)


class VocabChars:
    """The vocabulary's spelling on the device (include/sat_hip.h, sat_caption_chrf): ``word_offsets (V + 1) int32`` and ``word_chars
    (total) int32``, the code points of every id's word with whitespace stripped (``metrics.chrf_text``), and the host int
    ``max_word_chars``.  An id absent from ``vocab_itos`` spells ``<UNK>``, as ``SAT.itos`` does.  Built once and reused by every batch
    and trial: two copies to the device at construction, no launch and no device read afterwards."""

    def __init__(self, vocab_itos, vocab_size, device="cuda"):
        offsets, chars, self.max_word_chars = self.host_tables(vocab_itos, vocab_size)
        self.vocab_size, self.device = int(vocab_size), torch.device(device)
        if self.device.type != "cuda":
            raise L.SatHipError("sat_amd computes on the GPU only: VocabChars on %s (no CPU fallback)" % self.device)
        self.word_offsets = torch.from_numpy(offsets).to(self.device)
        self.word_chars = torch.from_numpy(chars if chars.size else np.zeros(1, np.int32)).to(self.device)     # never a null pointer

    @staticmethod
    def host_tables(vocab_itos, vocab_size):
        """``(word_offsets (V + 1) int32, word_chars (total) int32, max_word_chars)`` as numpy arrays on the host"""
        if int(vocab_size) < 1:
            raise ValueError("VocabChars: vocab_size=%d" % vocab_size)
        words = [metrics.chrf_text([str(vocab_itos.get(i, "<UNK>"))]) for i in range(int(vocab_size))]
        offsets = np.zeros(len(words) + 1, np.int64)
        np.cumsum([len(w) for w in words], out=offsets[1:])
        if offsets[-1] > np.iinfo(np.int32).max:
            raise ValueError("VocabChars: the vocabulary spells %d characters (int32 offsets)" % offsets[-1])
        chars = np.array([c for w in words for c in w], np.int32)
        return offsets.astype(np.int32), chars, max(len(w) for w in words)

    @classmethod
    def from_model(cls, model):
        return cls(model.hp.vocab_itos, model.hp.vocab_size, model.embedding.weight.device)


def chrf_scores(tokens, lengths, refs, ref_lengths, chars, beta=3.0, with_stats=False):
    """``(B,)`` float64 on the device, chrF per image (the maximum over its references), of hypotheses ``tokens (B, W)`` / ``lengths
    (B)`` against ``refs (B, R, T)`` / ``ref_lengths (B, R)`` (int32, on the device) over the spelling ``chars`` (a ``VocabChars``);
    ``with_stats``: also ``(B, R, 8)`` int32, per reference ``tp_1..tp_6, Lh, Lr`` (``metrics.chrf_stats``).  One launch."""
    L.require_gpu(tokens, lengths, refs, ref_lengths, chars.word_offsets, chars.word_chars)
    for t in (tokens, lengths, refs, ref_lengths):
        assert t.dtype == torch.int32 and t.is_contiguous()
    B, W = tokens.shape
    _, R, T = refs.shape
    scores = torch.empty(B, dtype=torch.float64, device=tokens.device)
    stats = torch.empty(B, R, 8, dtype=torch.int32, device=tokens.device) if with_stats else None
    L.check(L.lib().sat_caption_chrf(L.ptr(tokens), L.ptr(lengths), W, L.ptr(refs), L.ptr(ref_lengths), B, R, T, L.ptr(chars.word_offsets),
                                     L.ptr(chars.word_chars), chars.vocab_size, chars.max_word_chars, float(beta), L.ptr(scores), L.ptr(stats),
                                     L.stream_ptr()), "sat_caption_chrf")
    return (scores, stats) if with_stats else scores


def metrics_from_sums(counts, cosine_sum, perplexity_sum, images):
    """the seven keys of ``score_captions`` from host numbers: 12 summed integers, two float sums, the image count"""
    counts = [int(c) for c in counts]
    out = {k: metrics.bleu_from_stats(counts[0:4], counts[4:8], counts[8], counts[9], w) for k, w in BLEU_WEIGHTS.items()}
    out["cosine_similarity"] = float(cosine_sum) / images
    out["gleu"] = metrics.gleu_from_stats(counts[10], counts[11])
    out["perplexity"] = float(perplexity_sum) / images
    return out


def metrics_from_vector(v, images):
    """``metrics_from_sums`` of a host ``CaptionStats.vector()``: 14 numbers; 16 with the CIDEr-D and ROUGE-L sums; 15 or 17 with the
    chrF sum behind them (means over images)"""
    if len(v) not in (14, 15, 16, 17):
        raise ValueError("metrics_from_vector: %d numbers (14, 15, 16 or 17)" % len(v))
    out = metrics_from_sums(v[:12], v[12], v[13], images)
    if len(v) >= 16:
        out["cider"], out["rouge_l"] = float(v[14]) / images, float(v[15]) / images
    if len(v) in (15, 17):
        out["chrf"] = float(v[-1]) / images
    return out


def vector_keys(n):
    """the metric keys a ``CaptionStats.vector()`` of ``n`` numbers carries"""
    return METRIC_KEYS + (CONSENSUS_KEYS if n >= 16 else ()) + (CHRF_KEYS if n in (15, 17) else ())


class CaptionStats:
    """Sums over images: ``counts`` (12,) int64 (the columns of sat_caption_stats), ``cosine_sum`` / ``perplexity_sum`` (float64
    scalars) on the device, ``images`` a host int; scored against a ``ReferenceCorpus`` also ``consensus_sum`` (2,) float64, the sums of
    CIDEr-D and ROUGE-L; scored over a ``VocabChars`` also ``chrf_sum``, a float64 scalar; taken ``with_diversity`` also ``diversity``,
    a ``DiversityStats`` (it has a vector and ``metrics()`` of its own: ``vector()`` here does not carry it).  ``a + b`` adds;
    ``metrics()`` reads the device once."""

    def __init__(self, counts, cosine_sum, perplexity_sum, images, consensus_sum=None, chrf_sum=None, diversity=None):
        self.counts, self.cosine_sum, self.perplexity_sum, self.images = counts, cosine_sum, perplexity_sum, int(images)
        self.consensus_sum, self.chrf_sum, self.diversity = consensus_sum, chrf_sum, diversity

    def __add__(self, other):
        if (self.consensus_sum is None) != (other.consensus_sum is None):
            raise ValueError("CaptionStats: one side was scored against a ReferenceCorpus and the other was not")
        if (self.chrf_sum is None) != (other.chrf_sum is None):
            raise ValueError("CaptionStats: one side was scored with chrF (a VocabChars) and the other was not")
        if (self.diversity is None) != (other.diversity is None):
            raise ValueError("CaptionStats: one side carries diversity statistics (with_diversity) and the other does not")
        return CaptionStats(self.counts + other.counts, self.cosine_sum + other.cosine_sum, self.perplexity_sum + other.perplexity_sum,
                            self.images + other.images, None if self.consensus_sum is None else self.consensus_sum + other.consensus_sum,
                            None if self.chrf_sum is None else self.chrf_sum + other.chrf_sum,
                            None if self.diversity is None else self.diversity + other.diversity)

    def vector(self):
        """(14,) float64 on the device: the counts (exact below 2^53), then the two sums; (16,) with the CIDEr-D and ROUGE-L sums; the
        chrF sum, if any, comes last: (15,) or (17,)"""
        parts = [self.counts.to(torch.float64), self.cosine_sum.reshape(1), self.perplexity_sum.reshape(1)]
        if self.consensus_sum is not None:
            parts.append(self.consensus_sum.reshape(2))
        if self.chrf_sum is not None:
            parts.append(self.chrf_sum.reshape(1))
        return torch.cat(parts)

    def metrics(self):
        return metrics_from_vector(self.vector().cpu().tolist(), self.images)


@torch.no_grad()
def val_batch_stats(model, batch, beamk=3, max_gen_length=32, temperature=0.5, sample_method="beam", sample_topk=3, decoder_noise=None,
                    rescore_method=None, rescore_reward=0.5, seed=None, graph=False, corpus=None, topg=None, prefix=None, banned=None, no_unk=False,
                    sample_topp=0.9, chrf=None, chrf_beta=3.0, no_repeat_ngram=None, min_length=None, repetition_penalty=None, mbr_corpus=None,
                    mbr_reward=(1.0, 0.0), mbr_alpha=0.0, beam_groups=None, diversity_penalty=0.5, required=None, with_diversity=False):
    """``SAT.val_batch`` (model.py:684-691) as a ``CaptionStats``: search, selection, statistics and cosine enqueued back to back;
    with ``corpus`` (a ``ReferenceCorpus``) CIDEr-D and ROUGE-L against it in the same enqueue, with ``chrf`` (a ``VocabChars``) chrF
    with ``chrf_beta``.  ``topg`` / ``prefix`` / ``banned`` / ``no_unk`` constrain the search, ``no_repeat_ngram`` / ``min_length`` /
    ``repetition_penalty`` are its history rules (``SATDecoder.beam_decode_batched``).  ``rescore_method="MBR"`` reranks by consensus
    against ``mbr_corpus`` (``corpus`` when that is None) with ``mbr_reward`` / ``mbr_alpha``.  ``beam_groups`` / ``diversity_penalty``: the
    diverse beam search; ``required``: the words every caption must contain.  ``with_diversity``: the result carries ``.diversity``, a
    ``DiversityStats`` of the batch: ``sat_caption_diversity`` over every finished hypothesis of the same search buffers (the search
    is not run again; MBR's back-trace is reused) and the vocabulary usage of the selected captions: two or three more launches."""
    opt = constraints.SearchOptions.from_kwargs(locals())
    img, encoded_captions, lengths = batch
    dev = model.embedding.weight.device
    buffers, sel, ppl = _search_and_select(model, img.to(dev), opt, beamk, max_gen_length, temperature, rescore_method, rescore_reward, mbr_corpus, mbr_reward,
                                           mbr_alpha, corpus)
    tokens, lens = sel["tokens"], sel["lengths"]
    diversity = None
    if with_diversity:
        hyp_tokens, hyp_len = (sel["hyp_tokens"], sel["hyp_len"]) if "hyp_tokens" in sel else finished_hypotheses(buffers, model.pad_idx)
        V = model.embedding.weight.shape[0]
        diversity = DiversityStats(diversity_statistics(hyp_tokens, hyp_len, buffers["fin_count"]).sum(0, dtype=torch.int64),
                                   vocabulary_usage(tokens, lens, V).to(torch.int64), tokens.shape[0], V)
    refs = torch.as_tensor(encoded_captions).to(device=dev, dtype=torch.int32).contiguous()
    ref_lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
    stats, best = caption_statistics(tokens, lens, refs, ref_lengths, model.embedding.weight.detach().contiguous())
    consensus = None if corpus is None else consensus_scores(tokens, lens, refs, ref_lengths, corpus).sum(0)
    chrf_sum = None if chrf is None else chrf_scores(tokens, lens, refs, ref_lengths, chrf, chrf_beta).sum()
    return CaptionStats(stats.sum(0, dtype=torch.int64), best.sum(dtype=torch.float64), ppl.sum(dtype=torch.float64), tokens.shape[0], consensus,
                        chrf_sum, diversity)


def evaluate(model, loader, max_batches=None, seed=None, corpus=None, chrf=None, with_diversity=False, **decode):
    """``val_batch_stats`` over the batches of ``loader`` (at most ``max_batches``).  Returns ``{"batch_mean": the notebook's protocol,
    the plain mean of the per-batch metric dicts, "corpus": BLEU / GLEU taken once from the statistics summed over every image (cosine and
    perplexity: means over images), "batches", "images"}``.  The per-batch statistics stay on the device and are read once at the end.
    ``seed``: batch i of a sampled search draws with ``seed + i``.  ``corpus`` (a ``ReferenceCorpus``): both dicts gain "cider" and
    "rouge_l" (means over images), ``chrf`` (a ``VocabChars``; ``chrf_beta`` travels in ``decode``): both gain "chrf"; still one host
    read.  ``decode`` takes every keyword of ``val_batch_stats``, the search constraints
    ``topg`` / ``prefix`` / ``banned`` / ``no_unk``, the history rules ``no_repeat_ngram`` / ``min_length`` / ``repetition_penalty`` and
    ``rescore_method="MBR"`` with ``mbr_corpus`` (``corpus`` when that is None) / ``mbr_reward`` / ``mbr_alpha`` and the diverse beam search
    ``beam_groups`` / ``diversity_penalty`` among them.  ``with_diversity``: the result gains "diversity", ``metrics.diversity_from_stats`` of
    the sums over every image of the split (distinct-n, mBLEU, unique, hypotheses, vocabulary); the sums are added on the device batch
    by batch and read once, behind the metric vectors.  Without it the result and the launches are exactly those of before."""
    if corpus is not None:
        decode["corpus"] = corpus
    if chrf is not None:
        decode["chrf"] = chrf
    if with_diversity:
        decode["with_diversity"] = True
    vecs, images, diversity = [], [], None
    for i, batch in enumerate(loader):
        if max_batches is not None and i >= max_batches:
            break
        st = model.val_batch_stats(batch, seed=None if seed is None else int(seed) + i, **decode)
        vecs.append(st.vector()); images.append(st.images)
        if with_diversity:
            diversity = st.diversity if diversity is None else diversity + st.diversity
    if not vecs:
        raise ValueError("evaluate: the loader gave no batch")
    rows = torch.stack(vecs).cpu().tolist()                                  # the one host read
    per_batch = [metrics_from_vector(r, n) for r, n in zip(rows, images)]
    total = [sum(int(r[c]) for r in rows) for c in range(12)] + [sum(r[c] for r in rows) for c in range(12, len(rows[0]))]
    keys = vector_keys(len(rows[0]))
    out = {"batch_mean": {k: sum(d[k] for d in per_batch) / len(per_batch) for k in keys}, "corpus": metrics_from_vector(total, sum(images)),
           "batches": len(per_batch), "images": sum(images)}
    if with_diversity:
        out["diversity"] = diversity.metrics()                                # one more, at the end of the split (exact integers)
    return out


def draw_decode_params(rs, space=NOTEBOOK_SPACE):
    """one trial's parameters from ``rs`` (np.random.RandomState) in the notebook's order: choice, uniform, choice, choice, choice, uniform.
    An optional ``space["topgs"]`` (a list of top-g clipping widths, ``None`` = off) adds one more choice AFTER the notebook's draws and a
    ``topg`` entry; top-g clipping belongs to "beam" sampling, so a trial that drew another method carries ``topg=None``."""
    beamk = rs.choice(space["beamks"])
    temperature = rs.uniform(space["temperatures"][0], space["temperatures"][1])
    sample_method = rs.choice(space["sample_methods"])
    decoder_noise = rs.choice(space["decoder_noises"])
    rescore_method = rs.choice(space["rescore_methods"])
    rescore_reward = rs.uniform(space["rescore_rewards"][0], space["rescore_rewards"][1])
    row = {"beamk": int(beamk), "temperature": float(temperature), "sample_method": str(sample_method), "decoder_noise": float(decoder_noise),
           "rescore_method": str(rescore_method), "rescore_reward": float(rescore_reward)}
    if "topgs" in space:
        topgs = list(space["topgs"])
        topg = topgs[int(rs.randint(len(topgs)))]
        row["topg"] = int(topg) if topg is not None and row["sample_method"] == "beam" else None
    return row


def random_search(model, loader, trials, space=NOTEBOOK_SPACE, seed=None, max_batches=4, corpus=None, chrf=None, chrf_beta=3.0, mbr_corpus=None,
                  mbr_reward=(1.0, 0.0), mbr_alpha=0.0):
    """evaluate.ipynb's random search: ``trials`` draws from one ``np.random.RandomState(seed)``, each scored over the first
    ``max_batches`` batches.  Rows carry the notebook's 13 columns (the metrics are its batch means) plus ``<metric>_corpus``; with
    ``corpus`` (a ``ReferenceCorpus``, built once and reused by every trial) also cider, rouge_l, cider_corpus, rouge_l_corpus; with
    ``chrf`` (a ``VocabChars``, likewise) also chrf and chrf_corpus; with ``space["topgs"]`` also a ``topg`` column (``draw_decode_params``).
    ``"MBR"`` may stand in ``space["rescore_methods"]`` when ``mbr_corpus`` (or ``corpus``) is given: such a trial reranks by consensus
    with ``mbr_reward`` / ``mbr_alpha`` (its drawn ``rescore_reward`` is unused).  Without ``"MBR"`` in the space nothing changes."""
    with_mbr = "MBR" in list(space["rescore_methods"])
    if with_mbr and mbr_corpus is None and corpus is None:
        raise ValueError("random_search: 'MBR' in space['rescore_methods'] needs mbr_corpus (or corpus)")
    rs = np.random.RandomState(seed)
    rows = []
    extra = {} if corpus is None else {"corpus": corpus}
    if with_mbr:
        extra.update(mbr_corpus=mbr_corpus if mbr_corpus is not None else corpus, mbr_reward=mbr_reward, mbr_alpha=mbr_alpha)
    if chrf is not None:
        extra.update(chrf=chrf, chrf_beta=chrf_beta)
    for trial in range(int(trials)):
        row = draw_decode_params(rs, space)
        res = evaluate(model, loader, max_batches=max_batches, seed=None if seed is None else (int(seed) * 1000003 + trial) % (2 ** 62),
                       max_gen_length=space["max_gen_length"], **row, **extra)
        row.update({k: res["batch_mean"][k] for k in METRIC_KEYS})
        row.update({k + "_corpus": res["corpus"][k] for k in METRIC_KEYS})
        if corpus is not None:
            row.update({k: res["batch_mean"][k] for k in CONSENSUS_KEYS})
            row.update({k + "_corpus": res["corpus"][k] for k in CONSENSUS_KEYS})
        if chrf is not None:
            row.update({k: res["batch_mean"][k] for k in CHRF_KEYS})
            row.update({k + "_corpus": res["corpus"][k] for k in CHRF_KEYS})
        rows.append(row)
    return rows
